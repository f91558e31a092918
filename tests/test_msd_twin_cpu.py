"""workloads.MsdBlocks — the host twin and the definition of the displacement accumulator of the device MD loop (md_msd.inc) —
against a plain numpy statement of that definition over a stored trajectory; its statistics on independent Gaussian walkers
against the chi-square widths of the block means; the identities a rigid translation and a common drift must satisfy; and the
holder arithmetic and the fits of autoforce_amd.transport."""
import numpy as np
import pytest

SPECIES = [3, 15, 16]   # the model's table; 15 is absent from the frames below


def _plain(traj, numbers, masses, species, every, levels, com):
    """The definition, from the stored trajectory: per level the non-overlapping windows of 2^l samples."""
    samples = traj[::every]
    S = len(species)
    out = dict(count=np.zeros(levels, dtype=np.int64), msd=np.zeros((levels, S)), msd_sq=np.zeros((levels, S)), smd=np.zeros((levels, S)),
               smd_sq=np.zeros((levels, S)))
    for l in range(levels):
        lag = 1 << l
        for s in range(lag, len(samples), lag):
            d = samples[s] - samples[s - lag]
            if com:
                d = d - (masses[:, None] * d).sum(axis=0) / masses.sum()
            out["count"][l] += 1
            for k, z in enumerate(species):
                sel = numbers == z
                if not sel.any():
                    continue
                msd = (d[sel] ** 2).sum(axis=1).mean()
                smd = (d[sel].sum(axis=0) ** 2).sum() / sel.sum()   # (the reference's correlator)
                out["msd"][l, k] += msd
                out["msd_sq"][l, k] += msd * msd
                out["smd"][l, k] += smd
                out["smd_sq"][l, k] += smd * smd
    return out


@pytest.fixture(scope="module")
def stored():
    rng = np.random.default_rng(5)
    numbers = rng.permutation(np.array([3] * 300 + [16] * 41))   # (two chunks of the first species, a ragged one; unsorted)
    masses = np.where(numbers == 3, 6.94, 32.06) * (1.0 + 0.01 * rng.random(len(numbers)))
    traj = np.cumsum(rng.normal(size=(50, len(numbers), 3)) * 0.1 + 0.01, axis=0)
    return numbers, masses, traj


@pytest.mark.parametrize("com", [False, True])
@pytest.mark.parametrize("every", [1, 3])
def test_twin_is_the_definition(stored, every, com):
    from autoforce_amd.workloads import MsdBlocks
    numbers, masses, traj = stored
    tw = MsdBlocks(every, 5, com, masses, numbers, SPECIES)
    for x in traj:
        tw.add(x)
    got, want = tw.table(), _plain(traj, numbers, masses, np.array(SPECIES), every, 5, com)
    assert np.array_equal(got["count"], want["count"]) and got["count"][0] == (len(traj) - 1) // every
    assert np.array_equal(got["lags"], every * 2 ** np.arange(5)) and np.array_equal(got["n"], [300, 0, 41])
    assert got["samples"] == -(-len(traj) // every)
    for k in ("msd", "msd_sq", "smd", "smd_sq"):
        scale = np.abs(want[k]).max()
        print(every, com, k, np.abs(got[k] - want[k]).max() / scale)
        assert np.abs(got[k] - want[k]).max() <= 1e-12 * scale, k
        assert np.all(got[k][:, 1] == 0.0)          # (the absent species keeps zeros)
        assert np.all(got[k][want["count"] > 0][:, [0, 2]] > 0.0)


SIGMA, NZ, SAMPLES, LEVELS = 0.05, 500, 256, 5


@pytest.fixture(scope="module")
def walkers():
    """Independent Gaussian walkers, step variance SIGMA^2 per component and SAMPLE: one table per `every`."""
    from autoforce_amd.workloads import MsdBlocks
    out = {}
    for every in (1, 2):
        rng = np.random.default_rng(11 + every)
        tw = MsdBlocks(every, LEVELS, False, np.ones(NZ), np.full(NZ, 3), [3])
        x = np.zeros((NZ, 3))
        for n in range(SAMPLES * every):
            tw.add(x)
            x = x + rng.normal(size=(NZ, 3)) * (SIGMA / np.sqrt(every))
        out[every] = tw.table()
    return out


@pytest.mark.parametrize("every", [1, 2])
def test_walkers_within_the_chi_square_widths(walkers, every):
    """A window's msd is 3 sigma^2 lag chi2(3 n_z) / (3 n_z) and its smd 3 sigma^2 lag chi2(3) / 3: the mean of `count`
    independent windows has the relative widths sqrt(2 / (3 n_z count)) and sqrt(2 / (3 count)); six of them."""
    from autoforce_amd.transport import Msd
    tab = walkers[every]
    h = Msd(every, LEVELS).add(tab)
    lag = 2.0 ** np.arange(LEVELS)   # in samples
    assert np.array_equal(tab["count"], (SAMPLES - 1) // (2 ** np.arange(LEVELS)))
    rm = h.mean()["msd"][:, 0] / (3 * SIGMA ** 2 * lag)
    rs = h.mean()["smd"][:, 0] / (3 * SIGMA ** 2 * lag)
    print(every, rm - 1, rs - 1)
    assert np.all(np.abs(rm - 1) <= 6 * np.sqrt(2 / (3 * NZ * tab["count"])))
    assert np.all(np.abs(rs - 1) <= 6 * np.sqrt(2 / (3 * tab["count"])))
    # (the error bars are those widths, estimated from at least 15 windows: within a factor of two)
    rel = h.stderr()["msd"][:, 0] / h.mean()["msd"][:, 0] / np.sqrt(2 / (3 * NZ * tab["count"]))
    assert np.all((rel > 0.5) & (rel < 2.0)), rel


@pytest.mark.parametrize("every", [1, 2])
def test_diffusion_constants_of_walkers(walkers, every):
    """msd = 3 sigma^2 lag / every in evaluations of dt each: D = slope / 6 = sigma^2 / (2 every dt).  The slope of a weighted
    line is a linear form sum_l a_l y_l of the level means; its standard deviation under the weights of the chi-square widths is
    worked out below and is smaller than the width of the level with the fewest windows, whose six-fold is the margin."""
    from autoforce_amd.transport import Msd, diffusion_constants
    tab, dt = walkers[every], 2.0
    D = diffusion_constants(Msd(every, LEVELS).add(tab), dt)[3]
    want = SIGMA ** 2 / (2 * every * dt)
    for key, nz in (("Dt", NZ), ("Dj", 1)):
        width = np.sqrt(2 / (3 * nz * tab["count"]))      # relative, per level
        x = tab["lags"] * dt
        w2 = 1.0 / (x * width) ** 2
        xb = (w2 * x).sum() / w2.sum()
        a = w2 * (x - xb) / (w2 * (x - xb) ** 2).sum()    # slope = sum a y
        std = np.sqrt(((a * x * width) ** 2).sum())       # relative to the true slope
        print(every, key, D[key][0] / want - 1, std, width.max())
        assert std < width.max()
        assert abs(D[key][0] / want - 1) <= 6 * width.max()
        assert D[key][1] < D[key][0] < D[key][2] or key == "Dj"


def test_rigid_translation_and_common_drift(stored):
    from autoforce_amd.workloads import MsdBlocks
    numbers, masses, traj = stored
    # every atom moves by the same vector: |sum d|^2 / n = n |d|^2
    tw = MsdBlocks(1, 3, False, masses, numbers, SPECIES)
    shift = np.cumsum(np.random.default_rng(2).normal(size=(12, 1, 3)), axis=0)
    for s in shift:
        tw.add(traj[0] + s)
    t = tw.table()
    assert np.abs(t["smd"] - t["n"][None, :] * t["msd"]).max() <= 1e-12 * np.abs(t["smd"]).max() and t["msd"][0, 0] > 0
    # com: a drift common to all atoms changes nothing
    a, b = MsdBlocks(2, 4, True, masses, numbers, SPECIES), MsdBlocks(2, 4, True, masses, numbers, SPECIES)
    for n, x in enumerate(traj[:33]):
        a.add(x)
        b.add(x + n * np.array([0.3, -0.2, 0.05]))
    ta, tb = a.table(), b.table()
    for k in ("msd", "msd_sq", "smd", "smd_sq"):
        print(k, np.abs(ta[k] - tb[k]).max() / np.abs(ta[k]).max())
        assert np.abs(ta[k] - tb[k]).max() <= 1e-12 * np.abs(ta[k]).max(), k
    assert np.array_equal(ta["count"], tb["count"])


def test_holder_adds_tables(stored):
    from autoforce_amd.transport import Msd
    from autoforce_amd.workloads import MsdBlocks
    numbers, masses, traj = stored
    tabs = []
    for part in (traj[:20], traj[20:]):
        tw = MsdBlocks(1, 4, False, masses, numbers, SPECIES)
        for x in part:
            tw.add(x)
        tabs.append(tw.table())
    h = Msd(1, 4).add(tabs[0]).add(tabs[1])
    assert np.array_equal(h.count, tabs[0]["count"] + tabs[1]["count"])
    for k in ("msd", "msd_sq", "smd", "smd_sq"):
        assert np.array_equal(getattr(h, k), tabs[0][k] + tabs[1][k])
    win = np.concatenate([np.array([((p[s] - p[s - 1])[numbers == 3] ** 2).sum(axis=1).mean() for s in range(1, len(p))]) for p in (traj[:20], traj[20:])])
    assert abs(h.mean()["msd"][0, 0] - win.mean()) <= 1e-12 * win.mean()
    assert abs(h.stderr()["msd"][0, 0] - np.sqrt(win.var() / len(win))) <= 1e-9 * win.mean()
    with pytest.raises(ValueError):
        Msd(2, 4).add(tabs[0])
