"""CPU tests of workloads.pimd_baoab, the host twin and the definition of the ring-polymer loop (sgpr_md_pimd, md_pimd.inc): BAOAB
with the PILE-L thermostat around a small analytic calculator with the ASE surface — harmonic + quartic wells, five atoms of mixed
masses.  At one bead the twin is langevin_nvt, bit for bit; without forces and thermostat it is the exact free ring polymer; C is
orthonormal for every P; the scheme is of second order; the tables, the centroid-virial column and hbar are what they say."""
import math

import numpy as np
import pytest

from autoforce_amd.ase_shim import kB
from autoforce_amd.workloads import FS, HBAR, MASS, langevin_nvt, pimd_baoab, pimd_tables

NUMBERS = np.array([1, 3, 8, 15, 16])
CELL, PBC = 20.0 * np.eye(3), [True, True, True]
X0 = np.array([[2.0, 3.0, 4.0], [6.0, 5.0, 3.5], [9.0, 9.5, 8.0], [12.0, 4.0, 13.0], [15.0, 14.0, 6.0]])


class _Wells:
    """E = sum_i [ k_i |u_i|^2 / 2 + q |u_i|^4 / 4 ], u_i = x_i - X0_i; scale = 0: no forces at all."""
    implemented_properties = ["energy", "forces"]
    K, Q = np.array([5.0, 3.0, 8.0, 4.0, 6.0])[:, None], 2.0

    def __init__(self, scale=1.0):
        self.scale = scale

    def get_property(self, name, atoms=None):
        u = atoms.positions - X0
        r2 = (u * u).sum(1)[:, None]
        if name == "energy":
            return self.scale * float((0.5 * self.K * r2 + 0.25 * self.Q * r2 * r2).sum())
        return -self.scale * (self.K * u + self.Q * r2 * u)


def _start(P, seed=0, spread=0.05):
    rng = np.random.default_rng(seed)
    mass = np.array([MASS[int(z)] for z in NUMBERS])[:, None]
    beads = X0[None] + 0.1 * rng.normal(size=(1, 5, 3)) + spread * rng.normal(size=(P, 5, 3))
    vel = rng.normal(size=(P, 5, 3)) * np.sqrt(P * kB * 300.0 / mass)
    return beads, vel, mass


def _langevin(*a, **kw):
    """langevin_nvt's rows with copies of the arrays it goes on updating in place."""
    return [r[:4] + (r[4].copy(), r[5].copy()) for r in langevin_nvt(*a, **kw)]


def test_one_bead_is_langevin_nvt_bit_for_bit():
    beads, vel, _ = _start(1)
    kw = dict(temperature=300.0, dt_fs=0.5, friction=0.02)
    a = _langevin(_Wells(), NUMBERS, beads[0], CELL, PBC, 50, vel=vel[0], rng=np.random.default_rng(7), **kw)
    b = list(pimd_baoab(_Wells(), NUMBERS, beads, CELL, PBC, 50, vel=vel, rng=np.random.default_rng(7), **kw))
    assert len(a) == len(b) == 51
    for (step, E, Tk, _, pos, v), o in zip(a, b):
        assert o["n"] == step and o["energy"] == E
        assert np.array_equal(o["beads"][0], pos) and np.array_equal(o["velocities"][0], v)
    assert np.abs(b[-1]["beads"][0] - beads[0]).max() > 1e-3
    # ... and from the generator's own start: the same draws, the mean momentum removed
    a = _langevin(_Wells(), NUMBERS, beads[0], CELL, PBC, 5, rng=np.random.default_rng(8), **kw)
    b = list(pimd_baoab(_Wells(), NUMBERS, beads, CELL, PBC, 5, rng=np.random.default_rng(8), **kw))
    assert np.array_equal(b[-1]["beads"][0], a[-1][4]) and np.array_equal(b[-1]["velocities"][0], a[-1][5])


def _dft(P):
    """C by its formula, from numpy's vector functions and the unreduced argument: independent of pimd_tables' loops."""
    j, k = np.arange(P)[:, None], np.arange(P)[None, :]
    arg = 2.0 * np.pi * j * k / P
    C = np.where(2 * k < P, np.sqrt(2.0 / P) * np.cos(arg), np.sqrt(2.0 / P) * np.sin(arg))
    C[:, 0] = np.sqrt(1.0 / P)
    if P % 2 == 0:
        C[:, P // 2] = np.sqrt(1.0 / P) * (-1.0) ** np.arange(P)
    return C


@pytest.mark.parametrize("P", [2, 3, 8, 16, 32])
def test_free_ring_polymer_against_the_closed_form(P):
    T, dt_fs, steps = 600.0, 1.0, 37
    beads, vel, _ = _start(P, seed=P)
    rows = list(pimd_baoab(_Wells(0.0), NUMBERS, beads, CELL, PBC, steps, temperature=T, dt_fs=dt_fs, friction=0.0, pile_lambda=0.0, vel=vel))
    assert len(rows) == steps + 1 and not np.abs(rows[-1]["forces"]).any()
    C, t = _dft(P), steps * dt_fs * FS
    w = 2.0 * (P * kB * T / HBAR) * np.sin(np.arange(P) * np.pi / P)
    xt, vt = np.einsum("jk,jnc->knc", C, beads), np.einsum("jk,jnc->knc", C, vel)
    cs, sn = np.cos(w * t)[:, None, None], np.sin(w * t)[:, None, None]
    wk = w[:, None, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        xe = np.where(wk > 0.0, cs * xt + sn / wk * vt, xt + t * vt)
    ve = cs * vt - wk * sn * xt
    xe, ve = np.einsum("jk,knc->jnc", C, xe), np.einsum("jk,knc->jnc", C, ve)
    ex = np.abs(rows[-1]["beads"] - xe).max() / np.abs(xe).max()
    ev = np.abs(rows[-1]["velocities"] - ve).max() / np.abs(ve).max()
    print(f"P = {P}: w_max dt = {w.max() * dt_fs * FS:.3f}, relative error x {ex:.2e}, v {ev:.2e}")
    assert w.max() * dt_fs * FS > 0.3            # (dt does not have to resolve w_P: 2.5 at P = 16)
    assert ex <= 1e-11 and ev <= 1e-11


def test_C_is_orthonormal_for_every_P():
    worst = 0.0
    for P in range(1, 33):
        C = pimd_tables(P, kB * 300.0, FS, 1e-3, 1.0)["C"]
        worst = max(worst, np.abs(C.T @ C - np.eye(P)).max(), np.abs(C - _dft(P)).max())
    print("largest |C^T C - 1| or |C - formula|:", worst)
    assert worst <= 1e-14


def _hamiltonian(o, mass, P, T):
    wP = P * kB * T / HBAR
    d = o["beads"] - np.roll(o["beads"], -1, axis=0)
    return (0.5 * (mass[None] * o["velocities"] ** 2).sum() + 0.5 * wP * wP * (mass[None] * d * d).sum() + P * o["energy"])


def test_the_scheme_is_of_second_order():
    P, T = 8, 300.0
    beads, vel, mass = _start(P, seed=3)
    err = []
    for cut in (1, 2, 4):
        rows = list(pimd_baoab(_Wells(), NUMBERS, beads, CELL, PBC, 48 * cut, temperature=T, dt_fs=1.0 / cut, friction=0.0, pile_lambda=0.0, vel=vel))
        H = np.array([_hamiltonian(o, mass, P, T) for o in rows])
        err.append(np.abs(H - H[0]).max())
    ratios = [err[0] / err[1], err[1] / err[2]]
    print("max |H_P - H_P(0)| at dt, dt/2, dt/4:", err, "ratios", ratios)
    assert all(3.0 <= r <= 5.0 for r in ratios)


def test_tables_columns_and_constants():
    assert HBAR == 6.626070040e-34 / (2.0 * math.pi) / 1.6021766208e-19 * (1e10 * math.sqrt(1.6021766208e-19 / 1.660539040e-27))
    for P in (1, 2, 5, 32):
        tb = pimd_tables(P, kB * 450.0, 0.5 * FS, 2e-3, 0.7)
        one = tb["c1"] ** 2 + tb["c2"] ** 2
        assert np.abs(one - 1.0).max() <= np.finfo(float).eps
        assert tb["c1"][0] == math.exp(-2e-3 * 0.5 * FS) and tb["w"][0] == 0.0
        assert np.allclose(tb["c1"][1:], np.exp(-2.0 * 0.7 * tb["w"][1:] * 0.5 * FS), rtol=1e-14, atol=0.0)
        assert np.allclose(tb["w"], 2.0 * (P * kB * 450.0 / HBAR) * np.sin(np.arange(P) * np.pi / P), rtol=1e-14, atol=1e-300)
    # the sixteen scalars' columns 14 and 15, 12 and 13, 0 and 1 — each by its formula, independently of the twin's ordered sums
    P, T = 6, 300.0
    beads, vel, mass = _start(P, seed=11)
    rows = list(pimd_baoab(_Wells(), NUMBERS, beads, CELL, PBC, 4, temperature=T, dt_fs=0.5, friction=1e-2, vel=vel, rng=np.random.default_rng(2)))
    wP = P * kB * T / HBAR
    for o in rows:
        xbar = o["beads"].mean(axis=0)
        cv = 1.5 * 5 * kB * T - ((o["beads"] - xbar[None]) * o["forces"]).sum() / (2.0 * P)
        d = o["beads"] - np.roll(o["beads"], -1, axis=0)
        assert abs(o["cv"] - cv) <= 1e-12 * max(1.0, abs(cv))
        assert abs(o["spring"] - 0.5 * wP * wP * (mass[None] * d * d).sum()) <= 1e-12 * o["spring"]
        assert abs(o["mv2"] - (mass[None] * o["velocities"] ** 2).sum()) <= 1e-12 * o["mv2"]
        assert abs(o["mv2_pre"] - (mass[None] * o["velocities_pre"] ** 2).sum()) <= 1e-12 * o["mv2_pre"]
        assert abs(o["energy"] - o["energies"].mean()) <= 1e-12 * abs(o["energy"]) and o["cbead"] == 1
    assert rows[0]["mv2"] == rows[0]["mv2_pre"] and rows[1]["mv2"] != rows[1]["mv2_pre"]   # (no closing kick at the start)


def test_update_repeats_an_evaluation_with_nothing_moved():
    beads, vel, _ = _start(3)
    kw = dict(temperature=300.0, dt_fs=0.5, friction=1e-2, vel=vel)
    plain = list(pimd_baoab(_Wells(), NUMBERS, beads, CELL, PBC, 6, rng=np.random.default_rng(1), **kw))
    seen = []
    cut = list(pimd_baoab(_Wells(), NUMBERS, beads, CELL, PBC, 6, rng=np.random.default_rng(1), update=lambda o: seen.append(o["n"]) or o["n"] == 3, **kw))
    assert seen == list(range(7)) and len(cut) == 7
    for a, b in zip(plain, cut):
        assert np.array_equal(a["beads"], b["beads"]) and np.array_equal(a["velocities"], b["velocities"])
