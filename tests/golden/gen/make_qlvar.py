"""Generates tests/golden/g17_qlvar.npz by IMPORTING the reference's Qlvar (calculator/meta.py over descriptor/ql.py; read-only;
the stubs of this directory stand in for ase and mpi4py, as for make_meta.py).  Data only: per case on the golden g5_* frames the
Steinhardt Q_l of one atom, and its autograd gradients with respect to the positions [D, N, 3] and to the cell [D, 3, 3] — the
reference's colvar is fed a brute-force neighbour list (every image inside the model's rc = 6, by enumeration) through its own
interface get_neighbors(i) -> (indices, offsets), with xyz and cell that require grad.

    THEFORCE_REFERENCE=<checkout of the reference> python tests/golden/gen/make_qlvar.py

Reference call sites exercised (under theforce/): calculator/meta.py:81-108 (Qlvar); descriptor/ql.py:10-29 (Ql);
descriptor/cutoff.py:33-44 (PolyCut); descriptor/ylm.py (Ylm)."""
import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference tree

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(HERE, "stubs"), os.environ["THEFORCE_REFERENCE"]]   # a checkout of the reference (theforce)

import torch  # noqa: E402
import theforce  # noqa: E402,F401  (sets fp64 default)
from theforce.calculator.meta import Qlvar  # noqa: E402

RC = 6.0   # the cutoff of the golden models: what the calculator's list holds

# name -> (frame, index (None: the first atom of species i), i, j, cutoff, l)
CASES = {
    "si32_a0": ("g5_si32", 0, 14, 14, 4.0, [4, 6]),
    "si32_a5_images": ("g5_si32", 5, 14, 14, 6.0, [4]),
    "tric24_a0": ("g5_tric24", 0, None, 16, 6.0, [4, 6]),
    "tric24_last": ("g5_tric24", 23, None, 3, 6.0, [6]),
    "mixed64_zr_c4": ("g5_mixed64", None, 40, 8, 4.0, [4, 6]),
    "mixed64_zr_c6": ("g5_mixed64", None, 40, 8, 6.0, [4, 6]),
    "slab18_nearz": ("g5_slab18_nearz", 0, None, 29, 6.0, [4, 6]),
    "cluster16_a0": ("g5_cluster16", 0, None, 10, 6.0, [6]),
}


class BruteList:
    """Every neighbour image inside rc, by enumeration of the periodic images: get_neighbors(i) -> (indices, offsets)."""

    def __init__(self, x, cell, pbc, rc):
        self.x, self.cell, self.pbc, self.rc = x, cell, pbc, rc
        inv = np.linalg.inv(cell) if pbc.any() else np.zeros((3, 3))
        self.span = [int(np.ceil(rc * np.linalg.norm(inv[:, k]))) + 2 if pbc[k] else 0 for k in range(3)]
        self.inv = inv

    def get_neighbors(self, i):
        jj, off = [], []
        for j in range(len(self.x)):
            base = np.round((self.x[j] - self.x[i]) @ self.inv).astype(int) if self.pbc.any() else np.zeros(3, int)
            for s0 in range(-self.span[0], self.span[0] + 1):
                for s1 in range(-self.span[1], self.span[1] + 1):
                    for s2 in range(-self.span[2], self.span[2] + 1):
                        s = np.array([s0, s1, s2]) - np.where(self.pbc, base, 0)
                        if j == i and not s.any():
                            continue
                        if np.linalg.norm(self.x[j] - self.x[i] + s @ self.cell) < self.rc:
                            jj.append(j)
                            off.append(s)
        return np.array(jj, int), np.array(off, int).reshape(-1, 3)


def main():
    data = dict(names=np.array(sorted(CASES)), rc=np.array(RC))
    for name, (frame, index, zi, zj, cutoff, ls) in CASES.items():
        g = np.load(os.path.join(OUT, frame + ".npz"))
        numbers, x, cell, pbc = g["numbers"], g["positions"], g["cell"].reshape(3, 3), np.asarray(g["pbc"], bool)
        assert float(g["rc"]) == RC
        zi = int(numbers[index]) if zi is None else zi
        var = Qlvar(zi, zj, index=index, cutoff=cutoff, l=ls)
        xyz = torch.tensor(x, requires_grad=True)
        lll = torch.tensor(cell, requires_grad=True)
        nl = BruteList(x, cell, pbc, RC)
        q = var(numbers, xyz, lll, pbc, nl)
        gx, gc = np.zeros((len(ls), len(x), 3)), np.zeros((len(ls), 3, 3))
        for d in range(len(ls)):
            a, b = torch.autograd.grad(q[d], (xyz, lll), retain_graph=True, allow_unused=True)
            gx[d] = 0.0 if a is None else a.numpy()
            gc[d] = 0.0 if b is None else b.numpy()
        idx = int(var.index)
        jj, off = nl.get_neighbors(idx)
        env = numbers[jj] == zj
        r = np.linalg.norm(x[jj[env]] - x[idx] + off[env] @ cell, axis=1)
        data[f"{name}_frame"], data[f"{name}_index"], data[f"{name}_i"], data[f"{name}_j"] = np.array(frame), np.array(idx), np.array(zi), np.array(zj)
        data[f"{name}_cutoff"], data[f"{name}_l"] = np.array(cutoff), np.array(ls)
        data[f"{name}_Q"], data[f"{name}_dQdx"], data[f"{name}_dQdcell"] = q.detach().numpy(), gx, gc
        data[f"{name}_selected"] = np.array(int((r < cutoff).sum()))
        data[f"{name}_gap"] = np.array(float(np.abs(r - cutoff).min()))   # the nearest neighbour to the cutoff sphere
        print(name, "index", idx, "selected", int((r < cutoff).sum()), "Q", q.detach().numpy(), "gap to the sphere", data[f"{name}_gap"],
              "NaN in grad:", bool(np.isnan(gx).any() or np.isnan(gc).any()))
    np.savez_compressed(os.path.join(OUT, "g17_qlvar.npz"), **data)


if __name__ == "__main__":
    main()
