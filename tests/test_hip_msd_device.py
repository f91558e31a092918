"""GPU tests of the displacement accumulator of the device MD loop (sgpr_md_msd / sgpr_md_msd_read; md_msd_part_kernel and
md_msd_fold_kernel behind a sampled evaluation) against its host twin and definition workloads.MsdBlocks, bit for bit: the twin
is fed the positions of the SAME run's frame record at every = 1, so the accumulator is exercised beside the record.  One call
and a cut run, other settings, held components, Nose-Hoover, frames whose species segments end off a wave and span several
chunks, a covloss halt in the middle (the next_due guard and the speculative evaluation), a run that is not disturbed, what a
later run and the handle's memory owe to it, every refusal in both directions, and ActiveCalculator.run_md(msd=) on the device
against the host loop.  Frame, model, run loop and the bodies the six accumulators share: accumulator_device.py."""
import numpy as np
import pytest

import accumulator_device as A
from accumulator_device import _begin, _frame, _shared

pytestmark = pytest.mark.gpu

KEYS = ("count", "msd", "msd_sq", "smd", "smd_sq")


def _run(fr, msd, **kw):
    """accumulator_device.run with the accumulator `msd` = (every, levels, com) or None.  Returns (table or None, recorded
    positions [evals, N, 3] or None, scalar rows, final state)."""
    tabs, xs, rows, state = A.run(fr, *A.attached(msd=msd), label=f"accumulator {msd}", **kw)
    return tabs.get("msd"), xs, rows, state


def _twin(fr, msd, xs):
    from autoforce_amd.workloads import MsdBlocks
    tw = MsdBlocks(msd[0], msd[1], msd[2], fr[4], fr[0], _shared()[0].species)
    for x in xs:
        tw.add(x)
    return tw.table()


def _same(tab, want, what=""):
    print(f"{what}: count {list(tab['count'])} samples {tab['samples']} next_due {tab['next_due']} msd[0] device {list(tab['msd'][0])} "
          f"twin {list(want['msd'][0])} smd[-1] device {list(tab['smd'][-1])} twin {list(want['smd'][-1])}")
    for k in KEYS + ("lags", "species", "n"):
        assert np.array_equal(tab[k], want[k]), (what, k, np.abs(np.asarray(tab[k], float) - want[k]).max())
    assert tab["samples"] == want["samples"] and tab["next_due"] == want["next_due"], (what, tab["samples"], tab["next_due"])


ACC = A.Acc(name="msd", noun=b"displacements", moving_cell=b"a displacement in a moving cell mixes in the strain", polymer=b"centroid is",
            raw=lambda h, every=1, levels=4, com=0: A.lib().sgpr_md_msd(h, every, levels, com),
            detach=lambda h: A.lib().sgpr_md_msd(h, 0, 0, 0), read=lambda h: A.lib().sgpr_md_msd_read(h, None, None, None),
            py=lambda mdl: mdl.md_msd(1, 4), invalid=[dict(every=-1), dict(levels=0), dict(levels=33), dict(com=2)],
            port=29870, run=_run, twin=_twin, same=_same)


def test_one_call_and_a_cut_run_equal_the_twin():
    fr, msd = _frame(), (1, 5, False)
    tab, xs, rows, _ = _run(fr, msd)
    want = _twin(fr, msd, xs)
    assert list(want["count"]) == [39, 19, 9, 4, 2] and np.all(want["msd"] > 0.0) and np.all(want["smd"] > 0.0)
    _same(tab, want, "one call")
    tab2, xs2, rows2, _ = _run(fr, msd, cuts=(7, 1, 12, 20))
    assert np.array_equal(xs2, xs) and np.array_equal(rows2, rows)
    _same(tab2, want, "cut 7 + 1 + 12 + 20")


@pytest.mark.parametrize("variant", ["every3", "com", "held", "nose-hoover"])
def test_variants_equal_the_twin(variant):
    from fixed_common import mask
    fr = _frame()
    msd = (3, 3, False) if variant == "every3" else (1, 5, variant == "com")
    kw = dict(fixed=mask(len(fr[0]))) if variant == "held" else {}
    tab, xs, _, _ = _run(fr, msd, nh=(variant == "nose-hoover"), **kw)
    want = _twin(fr, msd, xs)
    if variant == "every3":
        assert list(want["count"]) == [13, 6, 3] and list(want["lags"]) == [3, 6, 12]
    if variant == "held":   # (a held component does not move: the twin sees d = 0 there, bit for bit)
        assert np.array_equal(xs[-1][kw["fixed"]], fr[1][kw["fixed"]])
    assert np.all(want["msd"] > 0.0)
    _same(tab, want, variant)


@pytest.mark.parametrize("kind", ["sub200", "chunks"])
def test_segments_off_a_wave_and_over_several_chunks(kind):
    from autoforce_amd.workloads import MSD_CHUNK
    fr, msd = _frame(kind), (1, 4, True)
    n = np.array([int(np.sum(fr[0] == z)) for z in _shared()[0].species])
    if kind == "sub200":
        assert n.min() < 64 and np.all(n % 64 != 0) and np.all(np.cumsum(n) % 64 != 0)
    else:
        assert MSD_CHUNK < n.max() < 2 * MSD_CHUNK and n.min() < 128
    tab, xs, _, _ = _run(fr, msd, cuts=(5, 11))
    want = _twin(fr, msd, xs)
    assert np.array_equal(want["n"], n) and np.all(want["msd"] > 0.0)
    _same(tab, want, kind)


def test_a_covloss_halt_counts_every_configuration_once():
    def halted(mid, k, xs):
        assert mid["count"][0] == k
    A.halt_counts_once(ACC, (1, 4, False), halted)


@pytest.mark.parametrize("nh", [False, True])
def test_the_accumulator_moves_nothing(nh):
    A.moves_nothing(ACC, nh, (2, 3, True), lambda tab: tab["count"][0] == 9)


def test_a_later_run_and_the_memory_owe_it_nothing():
    """accumulator_device.later_run_and_memory; the table is the run's (md_msd_table refuses the plain run), and the origins and
    the table go with the run."""
    def accumulate(mdl, fr):
        _begin(mdl, fr, seed=7)
        mdl.md_msd(1, 6, True)
        sc, code = mdl.md_run(10, None)
        assert code == 0 and mdl.md_msd_table()["count"][0] == 9

    def detach(mdl, fr, first):
        _begin(mdl, fr, seed=7)
        mdl.md_msd(1, 6, True)
    A.later_run_and_memory(ACC, accumulate, detach)


def test_a_detach_gives_the_memory_back_and_a_fresh_attach_starts_from_zeros():
    """md_msd(0, ...) on a begun run — before its first call and behind one — gives back exactly what the attach took (the way
    test_hip_vanhove_device.py's detach is checked), md_msd_table then refuses, and the next attach owes the table that went
    nothing: zeros before the first call, the twin's table behind a run."""
    from test_hip_teardown import _live
    mdl, fr, msd = _shared()[0], _frame(), (1, 6, True)
    _begin(mdl, fr, seed=7)
    mdl.md_msd(0, 0)                  # (the buffers of the run before are the handle's until a detach or md_end)
    plain = _live()
    mdl.md_msd(*msd)
    held = _live()
    assert held[0] > plain[0] and held[1] > plain[1]
    mdl.md_msd(0, 0)
    assert np.array_equal(_live(), plain)
    mdl.md_msd(*msd)
    assert np.array_equal(_live(), held)
    sc, code = mdl.md_run(6, None)
    assert code == 0 and mdl.md_msd_table()["count"][0] == 5
    running = _live()                 # (the call has sized the run's own buffers)
    mdl.md_msd(0, 0)
    print(f"live memory plain {list(plain)}, attached {list(held)}, behind a call {list(running)}, detached {list(_live())}")
    assert np.array_equal(running - _live(), held - plain)
    with pytest.raises(RuntimeError, match="no accumulator"):
        mdl.md_msd_table()
    _begin(mdl, fr, seed=7)
    mdl.md_record(1, velocities=False, results=False)
    mdl.md_msd(*msd)
    zero = mdl.md_msd_table()
    assert zero["samples"] == 0 and zero["next_due"] == 0 and not np.any(zero["count"])
    assert not any(np.any(zero[k]) for k in KEYS)
    sc, code = mdl.md_run(10, None)
    assert code == 0
    _same(mdl.md_msd_table(), _twin(fr, msd, mdl.md_frames()["positions"]), "a fresh attach behind a detach")


def test_refusals_in_both_directions_leave_the_handle_working():
    A.refusals(ACC)


def test_a_run_begun_on_two_ranks_refuses_the_accumulator_and_goes_on_working():
    A.two_rank_refusal(ACC)


def test_run_md_fills_equal_tables_on_the_device_and_through_the_host_loop(tmp_path):
    """accumulator_device.run_md_host_and_device with run_md(msd=holder), the host loop's MsdBlocks fed every step's positions:
    the same tables, bit for bit."""
    from autoforce_amd.transport import Msd, diffusion_constants
    tabs, holder, numbers = A.run_md_host_and_device(tmp_path, "msd", lambda cell: Msd(2, 4, True))
    print(f"counts {list(tabs[0]['count'])}, msd[0] host {list(tabs[0]['msd'][0])} device {list(tabs[1]['msd'][0])}")
    assert list(tabs[0]["count"]) == [20, 10, 5, 2]
    for k in KEYS + ("lags", "species", "n"):
        assert np.array_equal(tabs[0][k], tabs[1][k]), k
    D = diffusion_constants(holder, 1.0)
    assert set(D) == set(int(z) for z in np.unique(numbers)) and all(np.isfinite(v["Dt"][0]) for v in D.values())
