"""GPU tests of the callers of the nudged elastic band in the device loop: ActiveCalculator.run_neb on a calculator that learns
from nothing — the gate fires, the halting image goes to calculate(), the model grows, the optimizer is reset, the run ends
converged — against the host loop of the twin (workloads.neb_fire) around calculate() with the same updates and resets; and
cl.neb end to end on files, with `-i a.xyz 3 b.xyz` interpolation, relaxed ends, the path and the output band."""
import numpy as np
import pytest

import active_common as ac

pytestmark = pytest.mark.gpu

K = 3


def _images(seed=3, amp=0.12, jitter=0.02):
    rng0, numbers, pos, cell = ac.start(0)
    rng = np.random.default_rng(seed)
    end = pos + amp * rng.normal(size=pos.shape)
    R = np.array([pos + (i / (K + 1.0)) * (end - pos) + (jitter * rng.normal(size=pos.shape) if 0 < i < K + 1 else 0.0) for i in range(K + 2)])
    return numbers, R, cell


class _Frozen:
    """calculate() with the teacher detached: the prediction of the model as it stands, its covloss, no update — what one plain
    step of the device band computes for an image."""

    def __init__(self, calc):
        self.calc = calc

    def get_property(self, name, atoms=None):
        teacher, self.calc._calc = self.calc._calc, None
        try:
            return self.calc.get_property(name, atoms)
        finally:
            self.calc._calc = teacher

    def get_covloss(self):
        return self.calc.get_covloss()


def test_run_neb_on_the_device_equals_the_host_loop(tmp_path, monkeypatch):
    from autoforce_amd import SGPRModel
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.calculator import ActiveCalculator
    from autoforce_amd.workloads import PairTeacher, neb_fire
    monkeypatch.chdir(tmp_path)
    steps, fmax = 2000, 0.1
    numbers, R, cell = _images(amp=0.2, jitter=0.0)
    res = {}
    for mode in ("host", "device"):
        np.random.seed(11)
        teacher = PairTeacher(ac.SPECIES, rc=4.0)
        calc = ActiveCalculator(engine=SGPRModel(3, 3, 4, 4.5, species=ac.SPECIES), calculator=teacher, logfile=None, pckl=None, tape=None, **ac.KW)
        images = [Atoms(numbers, x, cell, True) for x in R]
        resets = []
        if mode == "host":
            images[1].calc = calc
            images[1].get_forces()                                   # the model is seeded on image 1, as run_neb does

            def update(o):   # the device loop's gate and what run_neb does behind it
                gate = calc._md_gate(numbers)
                if not (gate > 0.0 and o["covmax"].max() >= gate):
                    return None
                at = Atoms(numbers, o["band"][o["cimg"] - 1], cell, True)
                at.calc = calc
                size = calc.size
                calc.results = {}
                calc.calculate(at)
                if calc.size != size:
                    resets.append(o["n"])
                    return "reset"
                return "again"
            rows = list(neb_fire(_Frozen(calc), numbers, R, cell, True, steps, fmax, climb=True, species=calc.engine.species, update=update))
            last = (rows[-1]["band"], rows[-1]["energies"], rows[-1]["converged"], rows[-1]["n"] + 1)
        else:
            reset = calc.engine.neb_reset
            calc.engine.neb_reset = lambda: (resets.append(len(resets)), reset())[1]
            out = calc.run_neb(images, fmax=fmax, climb=True, steps=steps, chunk=16)
            assert calc.engine._md.get("neb") == K                   # the device loop has run
            last = (np.array([im.positions for im in images[1:-1]]), out["energies"], out["converged"], out["evaluations"])
            assert np.array_equal(images[0].positions, R[0]) and np.array_equal(images[-1].positions, R[-1])
        res[mode] = (last, teacher.calls, calc.size, len(resets))
        calc.engine.close()
    (hlast, hcalls, hsize, hres), (dlast, dcalls, dsize, dres) = res["host"], res["device"]
    print("evaluations", hlast[3], dlast[3], "teacher calls", hcalls, dcalls, "size", hsize, dsize, "resets", hres, dres)
    assert hcalls == dcalls and hsize == dsize and hres == dres and hlast[3] == dlast[3]
    assert dres >= 1 and dsize[1] > 2                                 # the model grew, the optimizer was reset behind it
    assert dlast[2] and hlast[2]                                      # the run ends converged
    assert np.array_equal(hlast[0], dlast[0]) and np.array_equal(hlast[1], dlast[1])
    assert np.abs(dlast[0] - R[1:-1]).max() > 1e-3                    # the band has moved


def test_run_neb_refuses_a_committee_and_mixed_constraints():
    from autoforce_amd import SGPRModel
    from autoforce_amd.ase_shim import Atoms, FixAtoms
    from autoforce_amd.calculator import ActiveCalculator
    from autoforce_amd.calculator_bcm import BCMActiveCalculator
    from autoforce_amd.workloads import PairTeacher
    numbers, R, cell = _images()
    images = [Atoms(numbers, x, cell, True) for x in R]
    bcm = BCMActiveCalculator(engine=SGPRModel(3, 3, 4, 4.5, species=ac.SPECIES), calculator=PairTeacher(ac.SPECIES, rc=4.0), logfile=None)
    with pytest.raises(NotImplementedError, match="committee"):
        bcm.run_neb(images)
    bcm.engine.close()
    calc = ActiveCalculator(engine=SGPRModel(3, 3, 4, 4.5, species=ac.SPECIES), calculator=PairTeacher(ac.SPECIES, rc=4.0), logfile=None, pckl=None,
                            tape=None, **ac.KW)
    images[2].set_constraint(FixAtoms(indices=[0]))
    with pytest.raises(NotImplementedError, match="different components"):
        calc.run_neb(images)
    calc.engine.close()


def test_neb_driver_end_to_end_on_files(tmp_path, monkeypatch):
    """cl.neb on files: two end structures, three images interpolated between them, the ends relaxed first (FIRE on the
    device), the band through run_neb; the path and the output band are extended XYZ with K + 2 frames per band."""
    from autoforce_amd import SGPRModel
    from autoforce_amd.calculator import ActiveCalculator
    from autoforce_amd.cl.md import read_frames
    from autoforce_amd.cl.neb import nudged_elastic_band, read_images
    from autoforce_amd.sgprio import Frame, format_extxyz
    from helpers import PairTeacher
    monkeypatch.chdir(tmp_path)
    np.random.seed(11)
    numbers, R, cell = _images(amp=0.2)
    wrapped = R[-1].copy()
    wrapped[5] += cell[0]                                            # an end image written with an atom in the next cell
    for name, x in (("a.xyz", R[0]), ("b.xyz", wrapped)):
        with open(name, "w") as f:
            f.writelines(format_extxyz(Frame(numbers, x, cell, [True] * 3, None, None, None)))
    images = read_images(["a.xyz", str(K), "b.xyz"])
    assert len(images) == K + 2
    for i, im in enumerate(images[1:-1], start=1):                   # linear in the minimum-image displacement
        np.testing.assert_allclose(im.positions, R[0] + (i / (K + 1.0)) * (R[-1] - R[0]), rtol=0, atol=1e-12)
    with pytest.raises(NotImplementedError, match="install ASE"):
        nudged_elastic_band(images, algo="BFGS")
    calc = ActiveCalculator(engine=SGPRModel(3, 3, 4, 4.5, species=ac.SPECIES), calculator=PairTeacher(rc=4.0), logfile=None, pckl=None,
                            tape=None, **ac.KW)
    calls = []
    run_neb = calc.run_neb
    calc.run_neb = lambda *a, **k: (calls.append(k), run_neb(*a, **k))[1]
    n_exact = nudged_elastic_band(images, fmax=0.1, climb=True, algo="FIRE", rel_if=1, algo_if="FIRE", trajectory="path.xyz", output="out.xyz",
                                  calc=calc)
    assert calls and calls[0]["climb"] and calc.engine._md.get("neb") == K
    assert n_exact >= 1 and calc.size[0] >= 1
    out = read_frames("out.xyz", ":")
    assert len(out) == K + 2
    for fr, im in zip(out, images):
        np.testing.assert_allclose(fr.positions, im.positions, rtol=0, atol=1e-12)
    assert all(fr.energy is not None and fr.forces is not None for fr in out[1:-1]) and out[0].energy is None
    path = read_frames("path.xyz", ":")
    assert len(path) >= K + 2 and len(path) % (K + 2) == 0
    np.testing.assert_allclose(path[-2].positions, out[-2].positions, rtol=0, atol=1e-12)   # the path ends with the output band
    assert np.abs(np.array([fr.positions for fr in out[1:-1]]) - np.array([fr.positions for fr in path[1:K + 1]])).max() > 1e-4
    calc.engine.close()
