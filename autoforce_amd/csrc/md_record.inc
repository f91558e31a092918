// md_record.inc — the frame record of the device loops (sgpr_md_record): a trajectory writer sees every `every`-th configuration
// of a run without the run being cut.  The reference writes its trajectory from the host loop, one calculator call per step
// (cl/md.py:24-26: `loginterval`, the writers attached at :117-128 and :155-166; the optimizers' trajectory= of cl/relax.py);
// here the loop stays on the device and, behind the last launch of a recorded evaluation, ONE more launch copies that
// configuration into a record in HBM, in caller atom order:
//     positions [N][3] | velocities_pre [N][3] (what the integrator holds: sgpr_md_state's) | packed [4N + 11]
// — exactly the values sgpr_md_state(which = -1) returns for configuration n had the call ended with that evaluation (the
// same slots of the rings, the same bits).  Positions and velocities live in sorted order on the device: the kernel reads
// them in that order (coalesced) and scatters rows of three doubles through the permutation; the species sort is stable, so
// the stores are runs of consecutive rows too.  `packed` is in caller order already: a straight copy.
//   The integrating kernels are not touched, and a run that records nothing launches what it launched before.
#pragma once

// One frame: element e of [0, max(3N, plen)) per thread.  x, v: the ring slots (sorted order; v null: not recorded), packed: the
// results' slot (null: not recorded), plen = 4N + 11.  Writes nothing once the run has halted BEFORE this evaluation (the halt
// word as md_nh_kernel and md_fire_move_kernel read it); whether the frame of the halting evaluation itself stands is the
// host's decision (sgpr_md_run: the covloss halt of an MD evaluation is known one evaluation late).
__global__ __launch_bounds__(256) void md_record_kernel(int N, int plen, const int *perm, const double *x, const double *v, const double *packed,
                                                        double *out_x, double *out_v, double *out_p, const int *halt, int step)
{
    if (*halt < step) return;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < 3 * N) {
        const int i = e / 3, k = e - 3 * i;
        const size_t o = 3 * (size_t)perm[i] + k;
        out_x[o] = x[e];
        if (v) out_v[o] = v[e];
    }
    if (packed && e < plen) out_p[e] = packed[e];
}
