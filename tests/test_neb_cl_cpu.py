"""CPU tests of the nudged-elastic-band driver (autoforce_amd/cl/neb.py) and of ActiveCalculator.run_neb's host loop — the twin
around calculate(), what runs where the device loop cannot — on the CPU engine: the reference's `-i` forms, interpolation in the
minimum-image displacement, the message for the reference's default optimizer without ASE, and a band that is learned on the
fly, converges and is written out."""
import numpy as np
import pytest

import active_common as ac
from helpers import OracleModel, PairTeacher

K = 3


def _ends(amp=0.2, seed=3):
    rng0, numbers, pos, cell = ac.start(0)
    end = pos + amp * np.random.default_rng(seed).normal(size=pos.shape)
    return numbers, pos, end, cell


def _write(name, numbers, x, cell):
    from autoforce_amd.sgprio import Frame, format_extxyz
    with open(name, "a") as f:
        f.writelines(format_extxyz(Frame(numbers, x, cell, [True] * 3, None, None, None)))


def test_the_reference_s_input_forms_and_interpolation(tmp_path, monkeypatch):
    from autoforce_amd.cl.neb import nudged_elastic_band, read_images
    monkeypatch.chdir(tmp_path)
    numbers, a, b, cell = _ends()
    wrapped = b.copy()
    wrapped[5] += cell[0] - cell[2]                                  # an end image written with an atom in another cell
    _write("a.xyz", numbers, a, cell)
    _write("b.xyz", numbers, wrapped, cell)
    images = read_images(["a.xyz", str(K), "b.xyz"])                 # -i first.xyz 3 last.xyz
    assert len(images) == K + 2
    np.testing.assert_allclose(images[0].positions, a, rtol=0, atol=1e-12)          # (the files hold sixteen digits)
    np.testing.assert_allclose(images[-1].positions, wrapped, rtol=0, atol=1e-12)
    for i, im in enumerate(images[1:-1], start=1):                   # linear in the minimum-image displacement
        np.testing.assert_allclose(im.positions, a + (i / (K + 1.0)) * (b - a), rtol=0, atol=1e-12)
        assert np.array_equal(im.numbers, numbers) and np.array_equal(im.cell, cell) and im.pbc.all()
    for x in (a, 0.5 * (a + b), b):
        _write("all.xyz", numbers, x, cell)
    np.testing.assert_allclose([im.positions[0, 0] for im in read_images(["all.xyz"])], [a[0, 0], 0.5 * (a[0, 0] + b[0, 0]), b[0, 0]],
                               rtol=0, atol=1e-12)                                # every frame of a file
    assert len(read_images(["a.xyz", "all.xyz", "b.xyz"])) == 5                                                       # explicit files
    with pytest.raises(NotImplementedError, match="install ASE"):
        nudged_elastic_band(images)                              # algo = 'BFGS', the reference's default


def test_neb_driver_on_the_cpu_engine(tmp_path, monkeypatch):
    """cl.neb end to end where the device loop is not available: run_neb takes the host loop (neb_fire around calculate()), the
    model learns on the way and the optimizer restarts behind it, the band converges, path and output are written."""
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.calculator import ActiveCalculator
    from autoforce_amd.cl.md import read_frames
    from autoforce_amd.cl.neb import interpolate, nudged_elastic_band
    monkeypatch.chdir(tmp_path)
    np.random.seed(11)
    numbers, a, b, cell = _ends()
    images = [Atoms(numbers, a, cell, True)] + [Atoms(numbers, a, cell, True) for _ in range(K)] + [Atoms(numbers, b, cell, True)]
    interpolate(images)
    teacher = PairTeacher(rc=4.0)
    calc = ActiveCalculator(engine=OracleModel(3, 3, 4, 4.5, species=ac.SPECIES), calculator=teacher, logfile=None, pckl=None, tape=None, **ac.KW)
    assert not calc.md_on_device_ok()
    fmax = 0.1
    n_exact = nudged_elastic_band(images, fmax=fmax, climb=True, algo="FIRE", rel_if=0, trajectory="path.xyz", output="out.xyz", calc=calc)
    assert n_exact >= 1 and n_exact == calc.size[0] and teacher.calls >= n_exact
    assert np.array_equal(images[0].positions, a) and np.array_equal(images[-1].positions, b)   # rel_if = 0: the ends stay
    out = read_frames("out.xyz", ":")
    assert len(out) == K + 2
    for fr, im in zip(out, images):
        np.testing.assert_allclose(fr.positions, im.positions, rtol=0, atol=1e-12)
    assert all(fr.energy is not None and fr.forces is not None for fr in out[1:-1]) and out[0].energy is None
    path = read_frames("path.xyz", ":")
    assert len(path) >= 2 * (K + 2) and len(path) % (K + 2) == 0
    # converged: the model's projected forces on the written band are below fmax (the plain forces are not: the band is no minimum)
    from autoforce_amd.workloads import neb_fire
    row = next(neb_fire(calc, numbers, np.array([im.positions for im in images]), cell, True, 0, fmax, climb=True, species=calc.engine.species))
    assert row["converged"] and row["gmax2"] < fmax * fmax
    assert max(np.sqrt((fr.forces ** 2).sum(axis=1).max()) for fr in out[1:-1]) > np.sqrt(row["gmax2"])
