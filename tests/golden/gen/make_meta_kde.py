"""Generates tests/golden/g16_meta_kde.npz by IMPORTING the reference's Meta and Gaussian_kde (read-only; the stubs of this
directory stand in for ase and mpi4py, as for make_meta.py).  Data only: per case (one and three dimensions) the deposits of a
confined walk in CV space — bins are revisited, so counts exceed one —, Gaussian_kde.histogram() after them (the reference's
merged-by-bin form of the hills: centres and counts), and Meta.energy at probe points with all the deposits counted, plain and
well-tempered.  Deposits and probes closer than 1e-4 sigma to a bin edge k sigma or a block edge k 5 sigma are drawn again (a
last-bit difference would move them by a bin); the test checks the margin of every point kept from these numbers alone.

    THEFORCE_REFERENCE=<checkout of the reference> python tests/golden/gen/make_meta_kde.py

Reference call sites exercised (under theforce/): calculator/meta.py:10-52 (Meta.__init__, energy); analysis/kde.py:11-75
(discrete, Gaussian_kde.__call__, count, histogram)."""
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
from theforce.calculator.meta import Meta  # noqa: E402

W, TEM, KEEP = 0.013, 900.0, 1e-4
CASES = {"k1": (1, 0.1, 300, 24), "k3": (3, np.array([0.1, 0.15, 0.2]), 400, 24)}   # name -> D, sigma, deposits, probes


def margin(c, sigma):
    u, u5 = c / sigma, c / (5.0 * sigma)
    return min(np.min(np.minimum(u - np.floor(u), np.ceil(u) - u)), 5.0 * np.min(np.minimum(u5 - np.floor(u5), np.ceil(u5) - u5)))


def main():
    rng = np.random.default_rng(20261020)
    data = dict(w=np.array(W), tem=np.array(TEM), names=np.array(sorted(CASES)))
    for name, (D, sigma, H, P) in CASES.items():
        sg = np.broadcast_to(np.asarray(sigma, float), (D,))
        c0 = rng.uniform(1.0, 3.0, size=D)
        dep, x, v = [], c0.copy(), np.zeros(D)
        while len(dep) < H:   # a damped walk around c0, a few sigma wide
            v = 0.7 * v + 0.6 * sg * rng.normal(size=D) - 0.15 * (x - c0)
            x = x + v
            if margin(x, sg) > KEEP:
                dep.append(x.copy())
        dep = np.array(dep)
        probes = []
        while len(probes) < P:
            q = dep[rng.integers(H)] + 1.5 * sg * rng.normal(size=D)
            if margin(q, sg) > KEEP:
                probes.append(q)
        probes = np.array(probes)
        tsig = float(sigma) if np.isscalar(sigma) else torch.tensor(sigma)
        plain, wt = Meta(None, sigma=tsig, w=W, tem=None), Meta(None, sigma=tsig, w=W, tem=TEM)
        for c in dep:
            plain.kde.count(torch.tensor(c))
            wt.kde.count(torch.tensor(c))
        hx, hw = plain.kde.histogram()
        data[f"{name}_sigma"] = np.asarray(sigma, float)
        data[f"{name}_deposits"], data[f"{name}_probes"] = dep, probes
        data[f"{name}_hist_x"], data[f"{name}_hist_w"] = hx.numpy().reshape(-1, D), hw.numpy()
        data[f"{name}_energy_plain"] = np.array([float(plain.energy(torch.tensor(q))) for q in probes])
        data[f"{name}_energy_wt"] = np.array([float(wt.energy(torch.tensor(q))) for q in probes])
        print(name, "D =", D, "deposits", H, "bins", len(hw), "largest count", hw.max().item(), "max V", data[f"{name}_energy_plain"].max())
    np.savez_compressed(os.path.join(OUT, "g16_meta_kde.npz"), **data)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        main()
