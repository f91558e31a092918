"""Generates tests/golden/g15_meta.npz by IMPORTING the reference's Meta, Posvar, Catvar and Gaussian_kde (read-only; the
stubs of this directory stand in for ase and mpi4py, as for make_golden.py).  Data only: an 8-atom, 3-species frame, a 200-step
random walk of it, and per step and case the collective variable, Meta.energy(cv) with the hills of the steps before it, and
its autograd gradient with respect to the positions — then the step deposits (Meta.update's kde.count), as
dyn.attach(meta.update) does in the reference's examples/meta-dyn/md.py.

    THEFORCE_REFERENCE=<checkout of the reference> python tests/golden/gen/make_meta.py

(it works in a temporary directory: Meta's constructor writes meta.hist)

Reference call sites exercised (under theforce/): calculator/meta.py:10-60 (Meta.__init__, energy), :63-79 (Posvar), :117-122
(Catvar); analysis/kde.py:12-69 (discrete, Gaussian_kde.__call__, count)."""
import os
import sys
import tempfile

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference tree

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(HERE, "stubs"), os.environ["THEFORCE_REFERENCE"]]   # a checkout of the reference (theforce)

import torch  # noqa: E402
import theforce  # noqa: E402,F401  (sets fp64 default)
from theforce.calculator.meta import Catvar, Meta, Posvar  # noqa: E402

STEPS = 200


def distance(i, j):
    def colvar(numbers, xyz, cell, pbc, nl):   # the reference docstring's example
        return (xyz[j] - xyz[i]).norm().view(1)
    return colvar


def cases():
    """name -> (colvar of the reference, the same as the twin's component list, sigma, tem)"""
    out = {}
    for tag, tem in (("plain", None), ("wt", 900.0)):
        out[f"d1_{tag}"] = (distance(0, 5), [("distance", 0, 5)], 0.1, tem)
        out[f"d3_{tag}"] = (Posvar(2), [("posvar", 2, None)], 0.08, tem)
        out[f"d4_{tag}"] = (Catvar(Posvar(1, select=8), distance(0, 7)), [("posvar", 1, 8), ("distance", 0, 7)], 0.1, tem)
    out["d3_vector_sigma"] = (Posvar(3, select=1), [("posvar", 3, 1)], np.array([0.05, 0.1, 0.2]), None)
    out["d3_lonely"] = (Posvar(7, select=40), [("posvar", 7, 40)], 0.1, None)   # the only atom of its species: the mean of nothing, n = 1
    return out


def main():
    rng = np.random.default_rng(20261019)
    numbers = np.array([1, 8, 1, 1, 8, 8, 1, 40])
    cell = np.array([[6.0, 0.0, 0.0], [0.5, 5.5, 0.0], [0.0, 0.3, 5.0]])
    x0 = rng.uniform(0.5, 4.5, size=(8, 3))
    # a walk that stays where it has been: the CVs revisit their bins and cross block edges
    walk = np.empty((STEPS, 8, 3))
    x, v = x0.copy(), np.zeros((8, 3))
    for n in range(STEPS):
        walk[n] = x
        v = 0.8 * v + 0.04 * rng.normal(size=(8, 3)) - 0.02 * (x - x0)
        x = x + v
    data = dict(numbers=numbers, cell=cell, walk=walk, w=np.array(0.013), names=np.array(sorted(cases())))
    nums = torch.tensor(numbers)
    lll = torch.tensor(cell)
    for name, (colvar, spec, sigma, tem) in cases().items():
        sg = sigma if np.isscalar(sigma) else torch.tensor(sigma)
        meta = Meta(colvar, sigma=sg, w=0.013, tem=tem)
        D = sum(1 if c[0] == "distance" else 3 for c in spec)
        cv, en, gr = np.empty((STEPS, D)), np.empty(STEPS), np.empty((STEPS, 8, 3))
        for n in range(STEPS):
            xyz = torch.tensor(walk[n], requires_grad=True)
            c = colvar(nums, xyz, lll, None, None)
            e = meta.energy(c)
            if torch.is_tensor(e) and e.grad_fn is not None:
                (g,) = torch.autograd.grad(e, xyz, allow_unused=True)
                gr[n] = 0.0 if g is None else torch.nan_to_num(g).numpy()
            else:
                gr[n] = 0.0
            cv[n], en[n] = c.detach().numpy(), float(e.detach()) if torch.is_tensor(e) else float(e)
            meta.kde.count(c.detach())
        data[f"{name}_cv"], data[f"{name}_energy"], data[f"{name}_grad"] = cv, en, gr
        data[f"{name}_sigma"] = np.asarray(sigma, float)
        data[f"{name}_tem"] = np.array(np.nan if tem is None else tem)
        data[f"{name}_spec"] = np.array([[0 if c[0] == "distance" else 1, c[1], -1 if c[2] is None else c[2]] for c in spec])
        print(name, "D =", D, "max V", en.max(), "max |grad|", np.abs(gr).max())
    # the format of meta.hist: the header and the lines Meta.update writes for the first three CVs of d4_plain
    colvar, spec, sigma, tem = cases()["d4_plain"]
    meta = Meta(colvar, sigma=sigma, w=0.013, tem=tem)
    meta.rank = 0
    for n in range(3):
        meta._cv = torch.tensor(data["d4_plain_cv"][n])
        meta.update()
    data["hist_text"] = np.array(open("meta.hist").read())
    np.savez_compressed(os.path.join(OUT, "g15_meta.npz"), **data)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        main()
