#!/usr/bin/env python3
"""Wall time per step of the Langevin device loop with and without one of its accumulators — `--which` msd (sgpr_md_msd), rdf
(sgpr_md_rdf), vacf (sgpr_md_vacf), vanhove (sgpr_md_vanhove), adf (sgpr_md_adf) or sq (sgpr_md_sq) — on the headline frame of bench.py (LiPS 4096
atoms, 512 inducing, fp64, deviates drawn on the device; --dims 32 32 16: 16384 atoms), taken in ONE process.  Path (a) is the plain
loop in calls of `--call` evaluations; the further paths of an accumulator are in its row of ROWS below: the device loop with the
accumulator in the settings worth comparing, and what a user had before it — md_record, the frames of every call fetched behind it
and fed to the accumulator's host twin in workloads.  Where the host pass takes seconds per configuration (all but msd) it runs
`--host-steps` steps (0 leaves it out: larger frames).  Every device path is warmed up first; then the paths alternate in `--rounds`
rounds of `--steps` steps, every window starting from the same frame.  The tables are read once at the end of a window, inside the
timing.  Prints one JSON line: microseconds per step of each path per round, medians, the differences to (a) per round, and whether
the device's tables equal the host twin's over the same steps (sq: agree within md_sq.inc's bound; its integers equal).

    python tools/accumulator_step_time.py --which rdf [--rounds 2] [--steps 2048] [--call 256] [--dims 16 | --dims 32 32 16 --host-steps 0]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from autoforce_amd import workloads as wl
from autoforce_amd.ase_shim import kB
from autoforce_amd.workloads import FS, MASS, fit_to_teacher, lips

ap = argparse.ArgumentParser()
ap.add_argument("--which", required=True, choices=("msd", "rdf", "vacf", "vanhove", "adf", "sq"))
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--steps", type=int, default=2048)
ap.add_argument("--call", type=int, default=256)
ap.add_argument("--warmup", type=int, default=256)
ap.add_argument("--dims", type=int, nargs="+", default=[16])
# (the accumulators' own settings: the defaults are in the rows)
for name, kind in (("host-steps", int), ("levels", int), ("rmax", float), ("bins", int), ("rmax-images", float), ("lags", int), ("rbins", int),
                   ("tbins", int), ("pbins", int), ("dmax", float), ("dbins", int), ("nq", int)):
    ap.add_argument("--" + name, type=kind, default=None)
args = ap.parse_args()

numbers, pos, cell, pbc = lips(args.dims[0] if len(args.dims) == 1 else tuple(args.dims), seed=0)
N = len(numbers)
mdl = bench.build_model(0, numbers, pos, cell, pbc, 512)
fit_to_teacher(mdl, numbers, pos, cell, pbc)
mass = np.array([MASS[int(z)] for z in numbers])
T, FRICTION = 300.0, 0.02
vel = np.random.default_rng(1).normal(size=(N, 3)) * np.sqrt(kB * T / mass[:, None])
BONDS = {(15, 16): 2.6, (3, 16): 3.0}   # (adf: P-S, Li-S; the other pairs never bond)
RC = float(mdl.cutoff)
frame = (numbers, mdl.species, cell, pbc)


def half_sphere(nq):
    """The nq shortest wave vectors of the cell's half-sphere (sq)."""
    from autoforce_amd.transport import q_vectors
    qmax = 1.0
    while True:
        hkl = q_vectors(cell, qmax, limit=1 << 30)
        if len(hkl) >= nq:
            return hkl[:nq]
        qmax *= 1.2


def sq_within(dev, host):
    """The device's tables within md_sq.inc's bound of the twin's, the integers equal."""
    B, F = wl.sq_bounds(np.abs(host["hkl"]).max(), host["smax"], host["n"], host["count"])
    return bool(np.array_equal(dev["count"], host["count"]) and dev["samples"] == host["samples"] and dev["next_due"] == host["next_due"]
                and np.all(np.abs(dev["f"] - host["f"]).max(axis=1) <= F) and np.all(np.abs(dev["mean"] - host["mean"]).max(axis=0) <= host["samples"] * B))


def vh(a, distinct):
    return (a.levels, a.rmax, a.rbins, a.tbins, a.pbins, a.dmax if distinct else None, a.dbins if distinct else 0)


def feed_velocities(twin, f):   # (vacf: the observer's velocity of a frame, from what the record holds)
    for n, v, F in zip(f["index"], f["velocities_pre"], f["forces"]):
        twin.add(wl.observer_velocities(v, F, mass, 0.5 * FS, 1 if n > 0 else 0))


# One row per accumulator.  defaults: its command-line settings; head: what of them the JSON line repeats; attach(every, **variant)
# and twin(**variant): the device accumulator and the host twin (fed the sampled configurations only); paths: the timed paths
# behind (a), each dict(every, host, steps (None: --steps; a host pass's own count, not warmed up), key (the table is kept under
# it), skip (untimed steps in front: vacf's ring fills first), once (timed once behind the rounds), further keywords: the
# variant); after: device runs behind the timing whose table is wanted; equal: (device key, host key) pairs over `keys`; minus:
# JSON key -> path, the differences to (a).
ROWS = dict(
    msd=dict(
        defaults=dict(levels=16, host_steps=0), head=lambda a: dict(levels=a.levels),
        attach=lambda every: mdl.md_msd(every, args.levels), twin=lambda: wl.MsdBlocks(1, args.levels, False, mass, numbers, mdl.species),
        paths=lambda a: dict(b_msd_every_step=dict(every=1, key="dev1"), c_msd_every_tenth=dict(every=10, key="dev10"),
                             d_record_and_host_pass_every_step=dict(every=1, host=True, key="host1"),
                             e_record_and_host_pass_every_tenth=dict(every=10, host=True, key="host10")),
        equal=(("dev1", "host1"), ("dev10", "host10")), keys=("count", "msd", "msd_sq", "smd", "smd_sq"),
        minus=dict(msd_every_step_minus_loop_us="b_msd_every_step", msd_every_tenth_minus_loop_us="c_msd_every_tenth")),
    rdf=dict(
        defaults=dict(host_steps=10, rmax=6.0, bins=120, rmax_images=24.0),
        head=lambda a: dict(rmax=a.rmax, bins=a.bins, rmax_images=a.rmax_images, host_steps=a.host_steps),
        attach=lambda every, rmax=None: mdl.md_rdf(every, rmax or args.rmax, args.bins),
        twin=lambda rmax=None: wl.RdfCounts(1, rmax or args.rmax, args.bins, 0.0, *frame),
        paths=lambda a: dict(b_rdf_every_step=dict(every=1), c_rdf_every_tenth=dict(every=10), d_rdf_images_every_tenth=dict(every=10, rmax=a.rmax_images),
                             e_record_and_host_pass_every_step=dict(every=1, host=True, steps=a.host_steps, key="host"),
                             f_record_and_host_pass_every_tenth=dict(every=10, host=True, steps=10 * max(1, a.host_steps // 5))),
        after=lambda a: [dict(every=1, steps=a.host_steps, key="device")], equal=(("device", "host"),), keys=("hist", "samples"),
        minus=dict(rdf_every_step_minus_loop_us="b_rdf_every_step", rdf_every_tenth_minus_loop_us="c_rdf_every_tenth")),
    vacf=dict(
        defaults=dict(host_steps=64, lags=256), head=lambda a: dict(lags=a.lags, host_steps=a.host_steps),
        attach=lambda every, origin_every=1: mdl.md_vacf(every, args.lags, origin_every),
        twin=lambda origin_every=1: wl.VacfRing(1, args.lags, origin_every, False, mass, numbers, mdl.species),
        record=dict(velocities=True, results=True), feed=feed_velocities,
        paths=lambda a: dict(b_vacf_every_step=dict(every=1), c_vacf_every_step_origin_16=dict(every=1, origin_every=16), d_vacf_every_tenth=dict(every=10),
                             e_record_and_host_pass_every_step=dict(every=1, host=True, steps=a.lags + a.host_steps, skip=a.lags, key="host", once=True)),
        after=lambda a: [dict(every=1, steps=a.lags + a.host_steps, key="device")], equal=(("device", "host"),),
        keys=("tracer", "collective", "count", "samples", "pending", "next_due"), minus_nested="minus_loop_us"),
    vanhove=dict(
        defaults=dict(host_steps=9, levels=10, rmax=4.0, rbins=80, tbins=6, pbins=8, dmax=6.0, dbins=120),
        head=lambda a: dict(levels=a.levels, rmax=a.rmax, bins=[a.rbins, a.tbins, a.pbins], dmax=a.dmax, dbins=a.dbins, host_steps=a.host_steps),
        attach=lambda every, distinct=False: mdl.md_vanhove(every, *vh(args, distinct)),
        twin=lambda distinct=False: wl.VanHoveCounts(1, *vh(args, distinct), *frame),
        paths=lambda a: dict(b_self_every_step=dict(every=1), c_self_and_distinct_every_step=dict(every=1, distinct=True),
                             d_self_and_distinct_every_tenth=dict(every=10, distinct=True),
                             e_record_and_host_pass_every_step=dict(every=1, distinct=True, host=True, steps=a.host_steps, key="host")),
        after=lambda a: [dict(every=1, distinct=True, steps=a.host_steps, key="device")], equal=(("device", "host"),),
        keys=("self", "over", "distinct", "count"),
        minus=dict(self_every_step_minus_loop_us="b_self_every_step", self_and_distinct_every_step_minus_loop_us="c_self_and_distinct_every_step",
                   self_and_distinct_every_tenth_minus_loop_us="d_self_and_distinct_every_tenth")),
    adf=dict(
        defaults=dict(host_steps=4, bins=180), head=lambda a: dict(rc=RC, bins=a.bins, host_steps=a.host_steps),
        attach=lambda every, cut=BONDS: mdl.md_adf(every, args.bins, cut), twin=lambda cut=BONDS: wl.AdfCounts(1, args.bins, cut, *frame),
        paths=lambda a: dict(b_adf_bonds_every_step=dict(every=1), c_adf_rc_every_step=dict(every=1, cut=RC), d_adf_bonds_every_tenth=dict(every=10),
                             e_record_and_host_pass_every_step=dict(every=1, host=True, steps=a.host_steps, key="host")),
        after=lambda a: [dict(every=1, steps=a.host_steps, key="device")], equal=(("device", "host"),), keys=("angles", "coord", "samples"),
        minus=dict(adf_bonds_every_step_minus_loop_us="b_adf_bonds_every_step", adf_rc_every_step_minus_loop_us="c_adf_rc_every_step",
                   adf_bonds_every_tenth_minus_loop_us="d_adf_bonds_every_tenth")),
    sq=dict(
        defaults=dict(host_steps=8, nq=2000, lags=64), head=lambda a: dict(nq=a.nq, lags=a.lags, host_steps=a.host_steps),
        attach=lambda every, lags=1: mdl.md_sq(every, half_sphere(args.nq), lags), twin=lambda lags=1: wl.SqRing(1, half_sphere(args.nq), lags, 1, *frame),
        paths=lambda a: dict(b_sq_every_step_one_lag=dict(every=1), c_sq_every_step_lags=dict(every=1, lags=a.lags), d_sq_every_tenth_one_lag=dict(every=10),
                             e_sq_every_tenth_lags=dict(every=10, lags=a.lags),
                             f_record_and_host_pass_every_step=dict(every=1, lags=a.lags, host=True, steps=a.host_steps, key="host")),
        after=lambda a: [dict(every=1, lags=a.lags, steps=a.host_steps, key="device")], equal=(("device", "host"),), compare=sq_within,
        minus=dict(sq_every_step_one_lag_minus_loop_us="b_sq_every_step_one_lag", sq_every_step_lags_minus_loop_us="c_sq_every_step_lags",
                   sq_every_tenth_one_lag_minus_loop_us="d_sq_every_tenth_one_lag", sq_every_tenth_lags_minus_loop_us="e_sq_every_tenth_lags")),
)
row = ROWS[args.which]
for k, v in row["defaults"].items():
    if getattr(args, k) is None:
        setattr(args, k, v)
tables = {}


def loop(steps, every=0, host=False, key=None, skip=0, **variant):
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, dt=FS, friction=FRICTION, kT=kB * T, seed=7)
    twin = None
    if every and host:
        mdl.md_record(every, **row.get("record", dict(velocities=False, results=False)))
        twin = row["twin"](**variant)
    elif every:
        row["attach"](every, **variant)
    done = timed_from = 0
    t0 = time.perf_counter()
    while done < steps:
        if skip and not timed_from and done >= skip:   # (the clock starts once every lag has an origin)
            timed_from, t0 = done, time.perf_counter()
        sc, code = mdl.md_run(min(args.call, (skip if done < skip else steps) - done), None)
        if code or not len(sc):
            raise RuntimeError(f"the device loop stopped with code {code} after {done} evaluations")
        done += len(sc)
        if twin is not None and mdl.md_frame_count():
            f = mdl.md_frames(closed=False, reuse=True)
            if "feed" in row:
                row["feed"](twin, f)
            else:
                for x in f["positions"]:
                    twin.add(x)
    if key:
        tables[key] = twin.table() if host else getattr(mdl, f"md_{args.which}_table")()
        if host and hasattr(twin, "smax"):   # (sq: what its bound takes)
            tables[key]["smax"] = twin.smax
    return (time.perf_counter() - t0) / (done - timed_from)


# (a host pass of its own step count runs only with --host-steps, and is not warmed up)
specs = {k: p for k, p in row["paths"](args).items() if args.host_steps or not (p.get("host") and "steps" in p)}
paths = {"a_loop": lambda s: loop(s)}
paths.update({k: (lambda s, p=p: loop(p.get("steps") or s, **{q: v for q, v in p.items() if q not in ("steps", "once")})) for k, p in specs.items()})
for k, f in paths.items():
    if k == "a_loop" or "steps" not in specs[k]:
        f(args.warmup)
rounds = {k: f for k, f in paths.items() if k == "a_loop" or not specs[k].get("once")}
times = {k: [] for k in rounds}
for _ in range(args.rounds):
    for k, f in rounds.items():
        times[k].append(1e6 * f(args.steps))
for k, f in paths.items():
    if k not in rounds:
        times[k] = [1e6 * f(args.steps)]
same = None
if all(h in tables for _, h in row["equal"]):
    for p in row.get("after", lambda a: [])(args):
        loop(p.pop("steps"), **p)
    if "compare" in row:
        same = bool(all(row["compare"](tables[d], tables[h]) for d, h in row["equal"]))
    else:
        same = bool(all(np.array_equal(tables[d][k], tables[h][k]) for d, h in row["equal"] for k in row["keys"]))
med = {k: float(np.median(v)) for k, v in times.items()}
minus = {j: [round(b - a, 2) for a, b in zip(times["a_loop"], times[k])] for j, k in row.get("minus", {}).items()}
if "minus_nested" in row:
    minus = {row["minus_nested"]: {k: [round(b - a, 2) for a, b in zip(times["a_loop"], times[k])] for k in list(rounds)[1:]}}
print(json.dumps(dict(atoms=N, inducing=512, **row["head"](args), rounds=args.rounds, steps=args.steps, call=args.call,
                      us_per_step={k: [round(t, 2) for t in v] for k, v in times.items()},
                      median_us={k: round(v, 2) for k, v in med.items()}, **minus, device_and_host_tables_equal=same)))
mdl.close()
