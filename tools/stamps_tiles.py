#!/usr/bin/env python3
"""Do the waves whose list is longer than one descriptor tile end later?  Builds the MD state that bench.py times (fit,
200 equilibration steps, 20 warm-up steps, then `extra` more), counts the atoms per list length from the list the library
returns, and splits the per-wave phase stamps of the LAST step's nl_fwd / desc_rev by list length.
Needs the -DSGPR_PHASE_STAMPS build (tools/build_stamps.sh):
  SGPR_HIP_LIB=$PWD/autoforce_amd/libsgpr_hip_stamps.so python3 tools/stamps_tiles.py [extra_steps] [out.json] [raw.npy]
(out.json: the figures printed; raw.npy: the per-wave records — atom, list length, forward stamps 0-5, reverse stamps 0-3; reverse stamp 3 is the head of the pair phase, reported as desc_rev_pairs_head =
cycles from stamp 1 to it)."""
import json
import os
import sys
import tempfile

os.environ["SGPR_STAMPS"] = "1"
dump = os.path.join(tempfile.mkdtemp(), "pstamps.txt")
os.environ["SGPR_PSTAMPS_FILE"] = dump
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench
from autoforce_amd.ase_shim import kB
from autoforce_amd.workloads import FS, MASS, fit_to_teacher, lips

extra = int(sys.argv[1]) if len(sys.argv) > 1 else 0
numbers, pos, cell, pbc = lips(16, seed=0)
N = len(numbers)
mdl = bench.build_model(0, numbers, pos, cell, pbc, 512)
fit_to_teacher(mdl, numbers, pos, cell, pbc)
mdl.set_weights(mdl.mu, choli=mdl.choli, vscale=mdl.make_vscale())
mass = np.array([MASS[int(z)] for z in numbers])
v0 = np.random.default_rng(11).normal(size=(N, 3)) * np.sqrt(kB * 600.0 / mass[:, None])
mdl.md_begin(numbers, pos, cell, pbc, mass, v0, dt=FS, friction=1e-3, kT=kB * 600.0, seed=11)
r0 = mdl.list_rebuilds()
sc, code = mdl.md_run(220 + extra, None)
assert code == 0 and len(sc) == 220 + extra, (len(sc), code)
r1 = mdl.list_rebuilds()
sc, code = mdl.md_run(1, None)   # the stamped step
last_rebuilt = mdl.list_rebuilds() != r1
ptr, _, _ = mdl.neighbors(N)
nn = np.diff(ptr)
out = {"steps": 221 + extra, "rebuilds": r1 - r0, "last_step_rebuilt": bool(last_rebuilt),
       "mean_neighbors": float(nn.mean()), "max_neighbors": int(nn.max()),
       "atoms_over_48": int((nn > 48).sum()), "atoms_over_64": int((nn > 64).sum())}
mdl.close()   # writes the per-wave records
rec = np.loadtxt(dump)   # ia, nn, forward stamps 0..5, reverse stamps 0..3
ia, wn = rec[:, 0].astype(int), rec[:, 1].astype(int)
fw, rv = rec[:, 2:8], rec[:, 8:12]
# reverse stamp 3, the head of the pair phase: tile 0's hand-over slot and length units are resolved (a wave without pair
# terms writes none)
headed = rv[:, 3] > rv[:, 1]
quad_two = np.zeros(len(ia), bool)
for q in range(0, len(ia), 4):
    quad_two[q:q + 4] = (wn[q:q + 4] > 48).any()
out["workgroups_with_atom_over_48_frac"] = float(quad_two[::4].mean())
for name, two in (("one_tile", wn <= 48), ("two_tile", wn > 48)):
    k = {"waves": int(two.sum())}
    if two.any():
        k["nl_fwd_list_filter"] = float((fw[two, 3] - fw[two, 0]).mean())
        k["nl_fwd_tiles"] = float((fw[two, 4] - fw[two, 3]).mean())
        k["nl_fwd_spectrum"] = float((fw[two, 5] - fw[two, 4]).mean())
        k["nl_fwd_wave_total"] = float((fw[two, 5] - fw[two, 0]).mean())
        k["desc_rev_phase_a"] = float((rv[two, 1] - rv[two, 0]).mean())
        k["desc_rev_pairs"] = float((rv[two, 2] - rv[two, 1]).mean())
        if (two & headed).any():
            k["desc_rev_pairs_head"] = float((rv[two & headed, 3] - rv[two & headed, 1]).mean())
        k["desc_rev_wave_total"] = float((rv[two, 2] - rv[two, 0]).mean())
    out[name + "_cycles"] = k
# s_memtime counts per CU (the 16 waves of a CU share a counter; the counters of different CUs are up to 1e12 apart, a
# few coincide to within 1e6): stamps compare only inside one CU.  Waves are clustered by their start values; every end
# is taken relative to the first start of its cluster, and clusters in which two CUs with near counters merged (span
# beyond 1e5 cycles: a launch lasts 3e4) are left out of the per-CU figures.
one, two = wn <= 48, wn > 48
for kname, start, end in (("nl_fwd", fw[:, 0], fw[:, 5]), ("desc_rev", rv[:, 0], rv[:, 2])):
    order = np.argsort(start)
    cuts = np.flatnonzero(np.diff(start[order]) > 1e6) + 1
    span_plain, span_two, n_merged = [], [], 0
    rel = np.full(len(ia), np.nan)
    for idx in np.split(order, cuts):
        r = end[idx] - start[idx].min()
        if r.max() > 1e5:
            n_merged += 1
            continue
        rel[idx] = r
        (span_two if two[idx].any() else span_plain).append(float(r.max()))
    ok = ~np.isnan(rel)
    k = {"clusters": len(cuts) + 1, "clusters_left_out": n_merged, "waves_compared": int(ok.sum()),
         "cu_span_without_two_tile_wave": {"n": len(span_plain), "mean": float(np.mean(span_plain)), "max": float(np.max(span_plain))},
         "cu_span_with_two_tile_wave": {"n": len(span_two), "mean": float(np.mean(span_two)) if span_two else None,
                                        "max": float(np.max(span_two)) if span_two else None}}
    for name, m in (("one_tile", one & ok), ("two_tile", two & ok)):
        if m.any():
            k[name + "_wave_end"] = {"n": int(m.sum()), "mean": float(rel[m].mean()), "p50": float(np.percentile(rel[m], 50)),
                                     "p90": float(np.percentile(rel[m], 90)), "max": float(rel[m].max())}
    out[kname + "_ends"] = k
if len(sys.argv) > 3:
    np.save(sys.argv[3], rec)
print(json.dumps(out, indent=1))
if len(sys.argv) > 2:
    json.dump(out, open(sys.argv[2], "w"), indent=1)
