"""Generates tests/golden/g20_vanhove.npz by IMPORTING the reference's TrajAnalyser (analysis/analysis.py; read-only; the stubs of
this directory stand in for ase and mpi4py, as for make_rdf.py — the two names of ase they lack, ase.io.Trajectory and
ase.neighborlist.natural_cutoffs, which analysis.py imports and this script never calls, are set on the stub modules here).  Data
only: a seeded random walk of 40 atoms in 3 species over 17 frames, one atom held still, and per case (bins of r, theta, phi) the
reference's own hist_rtp_displacements per (level, species) — called through a subclass whose __init__ takes the array of frames
and whose get_rand_pair walks the windows (k 2^l, (k + 1) 2^l) of level l in order, sample_size = the number of windows — with
the counts h N windows, asserted to be integers.

    THEFORCE_REFERENCE=<checkout of the reference> python tests/golden/gen/make_vanhove.py

The reference's `bins` counts edges: [rbins + 1, tbins + 1, pbins + 1].  `gap` is the smallest distance of any used (r, theta,
phi) to an edge of its axis and of r to rmax, over every window of every level: a condition on the inputs (>= 1e-9, asserted
here; change the bins of a case that fails it), so that the last bits of an arccos or an atan2 decide no bin.  The held atom has
d = 0 exactly — r = 0, theta = atan2(0, 0) = 0, phi = 0 sit ON edges by construction, np.histogramdd puts them in (0, 0,
pbins / 2) — and is left out of the gap.

Reference call sites exercised (under theforce/): analysis/analysis.py:22-35, 51-59 (TrajAnalyser.set_range, select), :178-210
(hist_rtp_displacements), :283-286 (Sampler); descriptor/sphcart.py:22-27 (cart_coord_to_sph)."""
import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference tree

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(HERE, "stubs"), os.environ["THEFORCE_REFERENCE"]]   # a checkout of the reference (theforce)

import ase.io  # noqa: E402
import ase.neighborlist  # noqa: E402

for mod, name in ((ase.io, "Trajectory"), (ase.neighborlist, "natural_cutoffs")):
    if not hasattr(mod, name):
        setattr(mod, name, None)

import theforce  # noqa: E402,F401  (sets fp64 default)
from theforce.analysis.analysis import TrajAnalyser  # noqa: E402
from theforce.descriptor.sphcart import cart_coord_to_sph  # noqa: E402

NUMBERS = np.array([3] * 17 + [15] * 9 + [16] * 14)
FRAMES, LEVELS, STEP, HELD, SIDE = 17, 4, 0.35, 5, 9.0
# name -> (rmax, rbins, tbins, pbins); "over" has displacements beyond rmax
CASES = {"rtp": (6.0, 16, 6, 8), "odd": (6.0, 12, 5, 7), "radial": (6.0, 10, 1, 1), "over": (1.1, 9, 4, 8)}


class Frame:
    """What hist_rtp_displacements touches of an Atoms."""

    def __init__(self, x):
        self.positions = x

    def get_volume(self):
        return SIDE ** 3


class Windows(TrajAnalyser):
    """TrajAnalyser over an array of frames; get_rand_pair walks the non-overlapping windows of the lag in order."""

    def __init__(self, frames, numbers):
        self.frames = [Frame(x) for x in frames]
        self.numbers = np.asarray(numbers)
        self.set_range(0, len(frames))
        self.k = 0

    def get_rand_pair(self, s, delta):
        a, b = self.frames[self.k * delta], self.frames[(self.k + 1) * delta]
        self.k += 1
        return a, b


def main():
    rng = np.random.default_rng(20)
    N = len(NUMBERS)
    steps = STEP * rng.normal(size=(FRAMES - 1, N, 3))
    steps[:, HELD] = 0.0
    x0 = SIDE * rng.random((N, 3))
    pos = np.concatenate([x0[None], x0[None] + np.cumsum(steps, axis=0)])
    species = np.unique(NUMBERS)
    traj = Windows(pos, NUMBERS)
    data = dict(names=np.array(sorted(CASES)), numbers=NUMBERS, species=species, positions=pos, levels=np.array(LEVELS), held=np.array(HELD),
                cell=np.diag([SIDE] * 3))
    for name, (rmax, rb, tb, pb) in sorted(CASES.items()):
        h = np.zeros((LEVELS, len(species), rb, tb, pb))
        counts = np.zeros(h.shape, dtype=np.int64)
        edges = [np.linspace(0, rmax, rb + 1), np.linspace(0, np.pi, tb + 1), np.linspace(-np.pi, np.pi, pb + 1)]
        gap = np.inf
        for l in range(LEVELS):
            windows = (FRAMES - 1) >> l
            for q, z in enumerate(species):
                traj.k = 0
                r, t, p, hh, rho = traj.hist_rtp_displacements(1 << l, rmax=rmax, bins=[rb + 1, tb + 1, pb + 1], select=int(z), sample_size=windows)
                assert traj.k == windows and hh.shape == (rb, tb, pb)
                nz = int(np.sum(NUMBERS == z))
                c = hh * nz * windows
                assert np.abs(c - np.round(c)).max() < 1e-9, (name, l, z)
                h[l, q], counts[l, q] = hh, np.round(c).astype(np.int64)
                assert np.isclose(rho, nz / SIDE ** 3)
            for k in range(windows):
                d = pos[(k + 1) << l] - pos[k << l]
                d = d[np.any(d != 0.0, axis=1)]
                rtp = np.array(cart_coord_to_sph(*d.T)).T
                use = rtp[:, 0] < rmax + 1e-6
                for ax in range(3):
                    v = rtp[:, ax] if ax == 0 else rtp[use, ax]
                    gap = min(gap, float(np.abs(v[:, None] - edges[ax][None, :]).min()))
        assert gap >= 1e-9, (name, gap)
        data[f"{name}_rmax"], data[f"{name}_bins"] = np.array(rmax), np.array([rb, tb, pb])
        data[f"{name}_h"], data[f"{name}_counts"], data[f"{name}_gap"] = h, counts, np.array(gap)
        print(name, "counts per level", counts.sum(axis=(1, 2, 3, 4)).tolist(), "of", [N * ((FRAMES - 1) >> l) for l in range(LEVELS)], "gap", gap)
    np.savez_compressed(os.path.join(OUT, "g20_vanhove.npz"), **data)


if __name__ == "__main__":
    main()
