"""Machine-learning accelerated nudged elastic band from the command line — theforce/cl/neb.py in this package's terms:

    python -m autoforce_amd.cl.neb -i images.xyz -o neb-out.xyz            # every frame of one file
    python -m autoforce_amd.cl.neb -i first.xyz 7 last.xyz                 # seven images interpolated in between
    python -m autoforce_amd.cl.neb -i a.xyz b.xyz c.xyz                    # explicit files; keywords from ./ARGS

The reference builds ase.neb.NEB(images, climb=climb, allow_shared_calculator=True) under an optimizer of ase.optimize
(`algo = 'BFGS'` by default), restarts that optimizer whenever the shared active calculator grew its model, and relaxes the two
end images with relax() first (`rel_if`, `algo_if`).  Here `algo = 'FIRE'` goes through ActiveCalculator.run_neb: FIRE on all
interior images at once with the band in device memory between model updates (md_neb.inc; workloads.neb_fire is the host twin
and the definition of the band: ASE's default `aseneb` method, spring constant 0.1).  `algo = 'BFGS'`, the reference's default
and therefore the default here, is ase.optimize.BFGS around ase.neb.NEB and asks for ASE, which is not part of this package;
`rel_if = 2` relaxes the ends once, as `rel_if = 1` does, and says so: the restarts happen inside run_neb with the ends fixed.
Interpolation is linear in the minimum-image displacement between the two end images, as NEB.interpolate(mic) does.  Images,
the path (`trajectory`: one band per batch of the run) and the optimised band (`output`) are extended XYZ; constraints travel in
the atoms objects handed to nudged_elastic_band (extended XYZ carries none).
  Neighbouring images must stay well inside half a cell of each other for every atom (workloads.neb_check_band): a band that
does not is refused at the start — add images."""
import argparse

import numpy as np

from . import gen_active_calc, get_default_args, read_args, update_args
from ..sgprio import Frame, format_extxyz
from .md import read_frames
from .relax import relax


def interpolate(images):
    """NEB.interpolate() on a list of atoms whose interior images are copies: positions linear between the first and the last
    image, in the minimum-image displacement (d - rint(d h^-1) h in the periodic directions)."""
    a, b = np.asarray(images[0].positions, float), np.asarray(images[-1].positions, float)
    cell, pbc = np.asarray(images[0].cell, float).reshape(3, 3), np.asarray(images[0].pbc, bool)
    d = b - a
    if pbc.any():
        s = d @ np.linalg.inv(cell)
        d = d - (np.where(pbc, np.rint(s), 0.0)) @ cell
    n = len(images) - 1
    for i in range(1, n):
        images[i].positions = a + (i / n) * d


def _write_band(f, images, energies=None, forces=None):
    for j, im in enumerate(images):
        e = None if energies is None or not (0 < j < len(images) - 1) else float(energies[j - 1])
        F = None if forces is None or not (0 < j < len(images) - 1) else forces[j - 1]
        f.writelines(format_extxyz(Frame(im.numbers, im.positions, im.cell, im.pbc, e, F, None)))
    f.flush()


def nudged_elastic_band(images, fmax=0.01, climb=False, algo="BFGS", rel_if=1, algo_if="BFGS", trajectory="neb-path.xyz", output="neb-out.xyz",
                        calc=None):
    """The keywords of theforce/cl/neb.py::nudged_elastic_band (same names and defaults; path and output are extended XYZ).
    images: a list of atoms objects; rel_if: relax the initial and final images: 0 (no), 1 (once), 2 (the reference: before every
    restart; here once, with a line that says so); algo_if: the optimizer of those relaxations (cl.relax.relax's algo).  Returns the number of exact (teacher) calculations."""
    if algo != "FIRE":
        # (the reference's loop — an ase.optimize class around ase.neb.NEB — is ASE's own and is not restated here)
        raise NotImplementedError(f"algo = '{algo}' is an ase.optimize class: install ASE; without it: ['FIRE'] "
                                  "(around ase.neb.NEB it is the reference's own driver, theforce/cl/neb.py; this one runs 'FIRE' on the device)")
    numbers = np.asarray(images[0].numbers)
    calc = gen_active_calc(species=sorted(set(int(z) for z in numbers))) if calc is None else calc
    load1 = calc.size[0]
    master = calc.rank == 0

    def relax_if(confirm):
        for i, label in ((0, "first"), (-1, "last")):
            if master:
                print(f"Relaxing the {label} image  ... ")
            relax(images[i], fmax=fmax, calc=calc, rattle=0.0, confirm=confirm, algo=algo_if, trajectory=f"relax_{label}.xyz")

    if rel_if:
        relax_if(confirm=True)
    path = open(trajectory, "w") if (trajectory and master) else None

    def on_band(n, st):
        for im, x in zip(images[1:-1], st["positions"]):
            im.positions = x
        _write_band(path, images, st["energy"], st["forces"])
    if master:
        print("(Re)starting NEB ...")
    # (run_neb restarts the optimizer itself whenever the model grew; rel_if = 2, a relaxation of the ends before every
    # restart, would move the ends under a band that is in device memory: the ends are relaxed once, and the user is told)
    if rel_if == 2 and master:
        print("rel_if = 2: the end images are relaxed once, before the band starts; they are not relaxed again at the restarts "
              "behind a model update (the band stays in device memory with fixed ends)")
    res = calc.run_neb(images, fmax=fmax, climb=climb, on_band=on_band if path is not None else None)
    if path is not None:
        path.close()
    load2 = calc.size[0]
    if master:
        print("\tNEB finished!" if res["converged"] else "\tNEB stopped before fmax was reached")
        print(f"\tTotal number of Ab initio calculations: {load2 - load1}\n")
        with open(output, "w") as f:
            _write_band(f, images, res["energies"], res["forces"])
    return load2 - load1


def read_images(args):
    """The reference's -i forms: files (every frame of each), a number between two files: that many copies of the last image
    read so far, to be interpolated."""
    from ..ase_shim import Atoms
    images, interp = [], False
    for a in args:
        if a.isdecimal():
            images.extend(images[-1].copy() for _ in range(int(a)))
            interp = True
        else:
            images.extend(Atoms(fr.numbers, fr.positions, fr.cell, fr.pbc) for fr in read_frames(a, ":"))
    if interp:
        interpolate(images)
    return images


def main(argv=None):
    ap = argparse.ArgumentParser(description="Machine Learning accelerated NEB.  It will also try to relax the initial and final images, "
                                             "thus there is no need for prior relaxation.")
    ap.add_argument("-i", "--images", default=["images.xyz"], nargs="*",
                    help="files for reading the images (extended XYZ): -i images.xyz OR -i file1 7 file2, which generates 7 images in "
                         "between, OR explicitly -i file1 file2 file3 ...")
    ap.add_argument("-o", "--output", default="neb-out.xyz", help="file for writing the optimized band (extended XYZ)")
    a = ap.parse_args(argv)
    images = read_images(a.images)
    kwargs = get_default_args(nudged_elastic_band)
    kwargs.pop("calc", None)
    update_args(kwargs, read_args())
    kwargs["output"] = a.output
    return nudged_elastic_band(images, **kwargs)


if __name__ == "__main__":
    main()
