"""Generates tests/golden/g19_rdf.npz by IMPORTING the reference's rdf (analysis/rdf.py; read-only; the stubs of this directory
stand in for ase and mpi4py, as for make_qlvar.py).  Data only: per case a two-frame "trajectory" — a golden g5_* frame and a
rattled copy — the reference's r axis, its g(r) for every pair it lists and the raw per-pair histograms.  The reference's function
is fed frames that implement only what it touches (numbers, tnumbers, get_volume(), update(cutoff), iteration over atoms) and
whose atoms are the reference's own descriptor.atoms.Local objects, built from a brute-force enumeration of every periodic image
within rmax (strictly), as make_qlvar.py feeds Qlvar.

    THEFORCE_REFERENCE=<checkout of the reference> python tests/golden/gen/make_rdf.py

`gap` is the smallest distance of any pair distance to a bin edge, to rmin and to rmax: a condition on the inputs (>= 1e-9,
asserted here; change `bins` of a case that fails it), so that the last bits of a distance decide no bin.

Reference call sites exercised (under theforce/): analysis/rdf.py:9-65 (get_numbers_pairs, rdf); descriptor/atoms.py:36-135
(Local, Local.select)."""
import itertools
import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference tree

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(HERE, "stubs"), os.environ["THEFORCE_REFERENCE"]]   # a checkout of the reference (theforce)

import torch  # noqa: E402
import theforce  # noqa: E402,F401  (sets fp64 default)
from theforce.analysis.rdf import rdf  # noqa: E402
from theforce.descriptor.atoms import Local  # noqa: E402

# name -> (frame, rmax, bins, rmin)
CASES = {f"{frame[3:]}_r{int(rmax)}": (frame, rmax, 32, 0.0)
         for frame in ("g5_mixed64", "g5_tric24", "g5_si32", "g5_slab18_nearz") for rmax in (4.0, 9.0)}
CASES["mixed64_r6_rmin"] = ("g5_mixed64", 6.0, 40, 1.5)
RATTLE = 0.08


def images(x, cell, pbc, rc):
    """Every (i, j, s) with (j, s) != (i, 0) and |x_j - x_i + s cell| < rc, by enumeration: per atom i (j [n], s [n, 3], d [n, 3])."""
    inv = np.linalg.inv(cell)
    span = [int(np.ceil(rc * np.linalg.norm(inv[:, k]))) + 2 if pbc[k] else 0 for k in range(3)]
    shifts = np.array(list(itertools.product(*[range(-n, n + 1) for n in span])))
    out = []
    for i in range(len(x)):
        base = np.where(pbc, np.round((x - x[i]) @ inv), 0.0).astype(int)                   # [N, 3] the nearest image of every j
        s = shifts[None, :, :] - base[:, None, :]                                           # [N, n_shifts, 3]
        d = (x - x[i])[:, None, :] + s @ cell
        r = np.linalg.norm(d, axis=2)
        ok = r < rc
        ok[i] &= s[i].any(axis=1)
        j, t = np.nonzero(ok)
        out.append((j, s[j, t], d[j, t]))
    return out


class Frame:
    """What theforce.analysis.rdf.rdf touches of a TorchAtoms."""

    def __init__(self, numbers, x, cell, pbc):
        self.numbers, self.x, self.cell, self.pbc = numbers, x, cell, pbc
        self.tnumbers = torch.from_numpy(numbers)
        self.loc = None

    def get_volume(self):
        return abs(np.linalg.det(self.cell))

    def update(self, cutoff):
        self.loc = [Local(i, j, self.numbers[i], self.numbers[j], torch.from_numpy(d), off=s)
                    for i, (j, s, d) in enumerate(images(self.x, self.cell, self.pbc, cutoff))]

    def __iter__(self):
        return iter(self.loc)


def main():
    data = dict(names=np.array(sorted(CASES)))
    rng = np.random.default_rng(19)
    for name, (frame, rmax, bins, rmin) in sorted(CASES.items()):
        g5 = np.load(os.path.join(OUT, frame + ".npz"))
        numbers, x, cell, pbc = g5["numbers"], g5["positions"], g5["cell"].reshape(3, 3), np.asarray(g5["pbc"], bool)
        xs = np.stack([x, x + RATTLE * rng.normal(size=x.shape)])
        frames = [Frame(numbers, xx, cell, pbc) for xx in xs]
        r, g = rdf(frames, rmax, bins=bins, rmin=rmin)
        pairs = list(g)
        # the raw histograms, through the reference's own Local.select and torch.histc as rdf() takes them
        hist = np.zeros((len(pairs), bins))
        for f in frames:
            for p, pair in enumerate(pairs):
                for loc, z in zip(f, f.numbers):
                    if z == pair[0]:
                        loc.select(*pair, bothways=True)
                        hist[p] += torch.histc(loc.r.pow(2).sum(dim=-1).sqrt(), bins=bins, min=rmin, max=rmax).numpy()
        assert np.array_equal(hist, np.round(hist))
        # every distance near the range, against the bin edges and the ends
        edges = rmin + (rmax - rmin) * np.arange(bins + 1) / bins
        gap = np.inf
        for xx in xs:
            for _, _, d in images(xx, cell, pbc, rmax + 1.0):
                rr = np.linalg.norm(d, axis=1)
                gap = min(gap, float(np.abs(rr[:, None] - edges[None, :]).min()))
        assert gap >= 1e-9, (name, gap)
        n = {int(z): int(np.sum(numbers == z)) for z in np.unique(numbers)}
        V = abs(np.linalg.det(cell))
        for p, (a, b) in enumerate(pairs):   # (the reference's g is its histogram over its own normalisation)
            want = hist[p] / (len(xs) * n[int(a)] * 4 * np.pi * r.numpy() ** 2 * float(r[1] - r[0]) * n[int(b)] / V)
            assert np.allclose(g[(a, b)].numpy(), want, rtol=1e-12, atol=0.0), (name, a, b)
        data[f"{name}_frame"], data[f"{name}_rmax"], data[f"{name}_rmin"], data[f"{name}_bins"] = np.array(frame), np.array(rmax), np.array(rmin), np.array(bins)
        data[f"{name}_positions"], data[f"{name}_r"] = xs, r.numpy()
        data[f"{name}_pairs"] = np.array([[int(a), int(b)] for a, b in pairs])
        data[f"{name}_g"] = np.stack([g[pair].numpy() for pair in pairs])
        data[f"{name}_hist"] = hist.astype(np.int64)
        data[f"{name}_gap"] = np.array(gap)
        print(name, "pairs", pairs, "counts", hist.sum(axis=1).astype(int).tolist(), "gap", gap, "finite g:", bool(np.isfinite(data[f"{name}_g"]).all()))
    np.savez_compressed(os.path.join(OUT, "g19_rdf.npz"), **data)


if __name__ == "__main__":
    main()
