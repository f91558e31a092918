"""What the tests of held atoms and components share: a toy calculator of elementwise arithmetic only (no library call whose
rounding could depend on the machine), short walks of the three host twins around it — test_fixed_twin_cpu.py holds them to
tests/golden/fixed_twins_unmasked.npz, recorded by tests/golden/gen/make_fixed_twins.py —, and a mask that mixes whole atoms
with single components.  Imports nothing that the commit before `fixed=` did not have."""
import numpy as np

from autoforce_amd.workloads import fire_relax, langevin_nvt, nose_hoover_nvt
from test_npt_twin_cpu import _system


class Springs:
    """Every atom in a harmonic well around its site, a stress proportional to the strain of the cell: +, -, * only."""
    implemented_properties = ["energy", "forces", "stress", "free_energy"]

    def __init__(self, sites, cell, k=1.5, kc=0.02):
        self.sites, self.cell, self.k, self.kc = np.array(sites, float), np.array(cell, float), k, kc
        self.results = {}

    def get_property(self, name, atoms=None):
        d = atoms.positions - self.sites
        sq = d * d
        e = 0.0
        for row in sq:                      # (a plain left-to-right sum)
            e = e + ((row[0] + row[1]) + row[2])
        s = self.kc * (np.asarray(atoms.cell, float) - self.cell)
        self.results = dict(energy=0.5 * self.k * e, forces=-self.k * d, free_energy=0.5 * self.k * e,
                            stress=np.array([s[0, 0], s[1, 1], s[2, 2], 0.5 * (s[1, 2] + s[2, 1]), 0.5 * (s[0, 2] + s[2, 0]), 0.5 * (s[0, 1] + s[1, 0])]))
        return self.results[name]


def toy():
    numbers, pos, cell, mass, v = _system(shear=True)
    sites = pos + 0.08 * np.random.default_rng(5).normal(size=pos.shape)
    return numbers, pos, cell, v, Springs(sites, 0.97 * cell)


def walks(**kw):
    """Short walks of the three twins around Springs; kw goes to every twin (nothing: the call of the commit before fixed=)."""
    numbers, pos, cell, v, calc = toy()
    pbc = [True] * 3
    out = {}
    rows = [(E, T, p.copy(), w.copy()) for _, E, T, _, p, w in langevin_nvt(calc, numbers, pos, cell, pbc, 25, 300.0, 1.0, 0.05, seed=3, vel=v, **kw)]
    out["lv_E"], out["lv_T"] = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    out["lv_x"], out["lv_v"] = rows[-1][2], rows[-1][3]
    rows = [(E, T, p.copy(), w.copy(), z, zi) for _, E, T, _, p, w, z, zi in nose_hoover_nvt(calc, numbers, pos, cell, pbc, 25, 300.0, 1.0, 20.0, vel=v, **kw)]
    out["nh_E"], out["nh_T"] = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    out["nh_x"], out["nh_v"] = rows[-1][2], rows[-1][3]
    out["nh_zeta"], out["nh_zint"] = np.array([r[4] for r in rows]), np.array([r[5] for r in rows])
    for tag, cr in (("fp", False), ("fc", True)):
        rows = list(fire_relax(calc, numbers, pos, cell, pbc, 25, 1e-9, cell_relax=cr, **kw))
        out[tag + "_E"] = np.array([r["energy"] for r in rows])
        out[tag + "_g"] = np.array([r["gmax2"] for r in rows])
        out[tag + "_P"] = np.array([r["P"] for r in rows])
        out[tag + "_dt"] = np.array([r["dt"] for r in rows])
        out[tag + "_x"], out[tag + "_h"] = np.array(rows[-1]["positions"]), np.array(rows[-1]["cell"])
    return out


def mask(N, seed=7):
    """Whole atoms (a quarter of them) and single components of others."""
    rng = np.random.default_rng(seed)
    fx = np.zeros((N, 3), bool)
    idx = rng.permutation(N)
    fx[idx[:N // 4]] = True
    fx[idx[N // 4:N // 4 + 3], 0] = True
    fx[idx[N // 4 + 3:N // 4 + 5], 2] = True
    fx[idx[N // 4 + 5], 1:] = True
    return fx
