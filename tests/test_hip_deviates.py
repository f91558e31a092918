"""GPU tests of the device loop's random stream (md_deviate in api.hip, read through sgpr_md_deviates) against its host twin
workloads.md_deviate, which tests/test_deviate_twin_cpu.py holds to the published vectors of Philox4x32-10: seeds and
configuration indices on both sides of 2^32 (the high words of key and counter), every (row, atom, component) of a frame
whose N is no multiple of a wave, a request longer than md_deviates_kernel's grid (its loop's second trip), one stretch
fetched in three calls, and the refusals.

Tolerance.  The integer part — Philox, the two 53-bit uniforms — is exact on both sides: u1 and u2 agree or the deviate is
off by O(1).  What is left are log, sqrt, cos and one product on the device against the host's; with log and sqrt good to
about one unit in the last place, cos to about two and the angle fl(tau u2) < 2 pi, a deviate is within roughly 10 units of
2^-52 r of its exact value, r = sqrt(-2 ln u1).  Allowed: 16 units per deviate, r from the twin (at most 3.1e-14).  Measured:
the twin against mpmath at 40 digits at most 2.08 units (on the CPU, test_deviate_twin_cpu.py); the device against the twin
at most 1.78 units over every case of this file (on the MI355X: below one unit in every case of a few hundred deviates, 1.772
over the 262 272 of the request longer than the grid)."""
import numpy as np
import pytest

from test_hip_md import _model

pytestmark = pytest.mark.gpu

UNITS = 16.0
M32 = (1 << 32) - 1


def _begin(mdl, frame, seed=1):
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS, MASS
    numbers, pos, cell, pbc = frame
    mass = np.array([MASS[int(z)] for z in numbers])
    mdl.md_begin(numbers, pos, cell, pbc, mass, None, dt=FS, friction=0.05, kT=kB * 600.0, seed=seed)


@pytest.fixture(scope="module")
def run():
    """One 64-atom LiPS frame (three species, shuffled: caller order is not the sorted order) with a run begun."""
    mdl, frame = _model(side=4)
    assert len(set(frame[0].tolist())) == 3 and np.any(np.diff(frame[0]) < 0)
    _begin(mdl, frame)
    yield mdl, len(frame[0])
    mdl.close()


def _draw(mdl, seed, t_first, count):
    from autoforce_amd import _lib
    _lib.check(_lib.load().sgpr_md_seed(mdl.handle, seed))
    return mdl.md_deviates(t_first, count)


def _twin(seed, t_first, count, N):
    """(deviates [count, N, 3], r [count, N, 3]) of the host twin."""
    from autoforce_amd.workloads import box_muller, md_deviate_uniforms
    t = np.int64(t_first) + np.arange(count, dtype=np.int64)
    u1, u2 = md_deviate_uniforms(seed, t[:, None, None], np.arange(N)[None, :, None], np.arange(3)[None, None, :])
    return box_muller(u1, u2), np.sqrt(-2.0 * np.log(u1))


def _same_as_twin(got, seed, t_first, label, hint=None):
    count, N, _ = got.shape
    ref, r = _twin(seed, t_first, count, N)
    err = np.abs(got - ref)
    units = np.divide(err, 2.0 ** -52 * r, out=np.where(err > 0.0, np.inf, 0.0), where=r > 0.0)
    worst = tuple(int(i) for i in np.unravel_index(np.argmax(units), units.shape))
    print(f"{label}: {got.size} deviates, device against twin at most {units[worst]:.3f} units of 2^-52 r (at row, atom, comp = {worst}: "
          f"device {float(got[worst])!r}, twin {float(ref[worst])!r}, r {float(r[worst])!r})")
    bad = ~(err <= UNITS * 2.0 ** -52 * r)
    assert not bad.any(), (label, int(bad.sum()), worst, got[worst], ref[worst], hint(got) if hint and bad.any() else None)
    return float(units[worst])


@pytest.mark.parametrize("seed", [1, 77, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 64) - 1],
                         ids=["1", "77", "2^32-1", "2^32", "2^32+1", "2^63", "2^64-1"])
def test_seeds_on_both_sides_of_the_key_words(run, seed):
    """Both words of the key: seeds below 2^32, with a zero low word, and with the top bits set."""
    mdl, N = run
    got = _draw(mdl, seed, 0, 4)
    _same_as_twin(got, seed, 0, f"seed {seed:#x}")
    if seed > M32:   # a dropped high word shows even if the twin shared the fault: the stream of the low word alone is another
        low = seed & M32
        assert np.abs(got - _twin(low, 0, 4, N)[0]).max() > 1e-3
        if low:   # (the device refuses seed 0)
            assert not np.array_equal(got, _draw(mdl, low, 0, 4))


@pytest.mark.parametrize("t_first,count", [((1 << 31) - 2, 4), ((1 << 32) - 2, 4), ((1 << 40) + 5, 2), ((1 << 63) - 3, 3)],
                         ids=["2^31-2", "2^32-2", "2^40+5", "2^63-3"])
def test_configuration_indices_on_both_sides_of_the_counter_words(run, t_first, count):
    """Both words of the counter: across the sign bit of the low word, across the carry into the high word, far inside it, and
    up to the last index an int64 holds (t_first + row must not overflow).  Every row with t >= 2^32 also differs from the
    device's own row of t mod 2^32: a dropped high word fails even if the twin shared the fault.  (2^31 - 2 has no such row.)"""
    mdl, N = run
    got = _draw(mdl, 77, t_first, count)
    _same_as_twin(got, 77, t_first, f"t_first {t_first:#x}")
    for r in range(count):
        assert r == 0 or not np.array_equal(got[r], got[r - 1])
        if t_first + r > M32:
            assert not np.array_equal(got[r], mdl.md_deviates((t_first + r) & M32, 1)[0]), (t_first, r)


def test_rows_atoms_and_components():
    """out[r, a, c] is the twin at (t_first + r, a, c) for every atom and component of a 200-atom cut of the 512-atom frame
    (three waves and a part of one; caller order is not the sorted order)."""
    from autoforce_amd.workloads import md_deviate
    mdl, (numbers, pos, cell, pbc) = _model()
    keep = np.sort(np.random.default_rng(11).choice(len(numbers), size=200, replace=False))
    numbers, pos = numbers[keep], pos[keep]
    assert np.any(np.diff(numbers) < 0)
    _begin(mdl, (numbers, pos, cell, pbc), seed=77)
    t_first, count, N = 3, 5, len(numbers)
    got = mdl.md_deviates(t_first, count)
    assert got.shape == (count, N, 3)

    def hint(got):   # which transposed reading of the three indices the device matches, if any
        r, a, c = np.arange(count)[:, None, None], np.arange(N)[None, :, None], np.arange(3)[None, None, :]
        o = np.zeros((count, N, 3), dtype=np.int64)
        readings = {"atom and comp exchanged": md_deviate(77, t_first + r + o, c + o, a + o),
                    "row and atom exchanged": md_deviate(77, t_first + a + o, r + o, c + o),
                    "flattened as [N][count][3]": md_deviate(77, t_first + (r * N + a) % count + o, (r * N + a) // count + o, c + o)}
        return [k for k, v in readings.items() if np.abs(got - v).max() < 1e-9] or "none of the transposed readings"

    _same_as_twin(got, 77, t_first, "rows, atoms, components", hint)
    mdl.close()


def test_a_request_longer_than_the_grid(run):
    """count 3N = 262 272 deviates at N = 64, count = 1366: 128 more than the 1024 x 256 threads of md_deviates_kernel, so its
    loop takes a second trip.  The whole array against the twin (the carry into the counter's high word lies inside it), and
    its last rows — the second trip's — against a small call of their own, bit for bit."""
    mdl, N = run
    assert N == 64
    count = 1366
    assert 1024 * 256 < count * 3 * N <= 1024 * 256 + 3 * N
    t_first = (1 << 32) - 683
    got = _draw(mdl, 77, t_first, count)
    _same_as_twin(got, 77, t_first, "second trip of the grid")
    tail = mdl.md_deviates(t_first + count - 2, 2)
    assert np.array_equal(got[-2:], tail)
    assert (count - 1) * 3 * N < 1024 * 256   # (the last row is where the second trip begins)


def test_one_stretch_in_three_calls(run):
    """Rows [0, 7), [7, 8) and [8, 40) fetched separately have the bits of one call: the device against itself."""
    mdl, N = run
    whole = _draw(mdl, 77, 0, 40)
    parts = np.concatenate([mdl.md_deviates(0, 7), mdl.md_deviates(7, 1), mdl.md_deviates(8, 32)])
    assert np.array_equal(whole, parts)


def test_refusals_leave_the_handle_as_it_was():
    """No run begun, a run ended, seed 0, count 0 and count -1: SgprError with the library's words, nothing allocated, and the
    same bits afterwards."""
    from autoforce_amd import SgprError, _lib, live_device_memory
    mdl, frame = _model(side=4)
    lib, h, N = _lib.load(), mdl.handle, len(frame[0])
    out = np.full((2, N, 3), 7.0)
    no_run = "sgpr_md_deviates: call sgpr_md_begin and sgpr_md_seed first"

    def refused(t_first, count, words):
        mem = live_device_memory()
        with pytest.raises(SgprError, match=words):
            _lib.check(lib.sgpr_md_deviates(h, t_first, count, _lib.ptr(out)))
        assert live_device_memory() == mem and np.all(out == 7.0)

    _lib.check(lib.sgpr_md_seed(h, 77))
    refused(0, 2, no_run)                                     # seeded, no run begun
    _begin(mdl, frame, seed=77)
    bits = mdl.md_deviates(0, 2)
    _same_as_twin(bits, 77, 0, "before the refusals")
    mem0 = live_device_memory()
    _lib.check(lib.sgpr_md_seed(h, 0))
    refused(0, 2, no_run)                                     # a run, no seed
    _lib.check(lib.sgpr_md_seed(h, 77))
    refused(0, 0, "sgpr_md_deviates: bad arguments")
    refused(0, -1, "sgpr_md_deviates: bad arguments")
    assert np.array_equal(mdl.md_deviates(0, 2), bits) and live_device_memory() == mem0
    mdl.md_end()
    refused(0, 2, no_run)                                     # the run ended
    _begin(mdl, frame, seed=77)
    assert np.array_equal(mdl.md_deviates(0, 2), bits)
    mdl.close()
