/* tsu_hip_multispin_quench.h -- K9: real-space overlap correlations, two-time correlations and quench runs of a multispin-coded
 * glass (csrc/multispin_quench.hip).
 *
 * Part of the C ABI of libtsu_hip.so: included by tsu_hip.h after tsu_hip_multispin_corr.h (inside its extern "C" block); include
 * tsu_hip.h, not this file.  Its ctypes prototypes are tsu._hip.MULTISPIN_QUENCH_SIGNATURES, one to one.
 *
 * Contract ("Real-space correlations and quench runs of multispin-coded glasses (K9)").  The site field of
 * slot t and sample s is f = a b, the two replicas at the slot, or f = s with one replica.  For a periodic axis d of length L_d
 * and r = 0 .. L_d / 2, C_d[r] = sum_x f_x f_{x + r e_d} over all N sites with wrap-around: with X = a ^ b (or X = a) it is
 * N - 2 count(bits set in X_x ^ X_{x + r e_d}), per bit position.  Integers only, the same on every run; C_d[0] = N.  An open axis
 * has no correlator.  The two-time correlation of plane (t, a) against a stored snapshot is sum_x s_x(now) s_x(snap) =
 * N - 2 count(bits set in now ^ snap) per sample.  Pad bits are computed like any other bit (the outputs have 64 W columns).
 */
#ifndef TSU_HIP_MULTISPIN_QUENCH_H
#define TSU_HIP_MULTISPIN_QUENCH_H
#ifndef TSU_HIP_H
#error "include tsu_hip.h, which includes this header"
#endif

#define TSU_MSC_SNAPSHOT_SLOTS 8    /* snapshots a handle keeps at most, and waiting times of a quench run */
#define TSU_MSC_C4_MAX_AXIS 16382   /* the longest periodic axis tsu_msc_c4 takes: one line of it has to fit the LDS of a workgroup */

/* C_d[r] of the planes as they are, per periodic axis: c_z [n_temps][64 W][depth / 2 + 1], c_r [...][rows / 2 + 1],
 * c_c [...][cols / 2 + 1].  A pointer is NULL exactly when its axis is open (TSU_E_INVALID otherwise, and when no axis is
 * periodic); TSU_E_UNSUPPORTED for a periodic axis longer than TSU_MSC_C4_MAX_AXIS.  Works on any K9 handle, with or without
 * tempering or the modes switched on.  Synchronous. */
int tsu_msc_c4(tsu_msc* h, int64_t* c_z, int64_t* c_r, int64_t* c_c);
/* n = 0 .. TSU_MSC_SNAPSHOT_SLOTS device copies of all planes; 0 frees them.  The snapshots of the slots that stay are kept. */
int tsu_msc_snapshot_slots(tsu_msc* h, int n);
/* Copies the planes as they are into `slot` (device to device, on the handle's stream).  Asynchronous. */
int tsu_msc_snapshot(tsu_msc* h, int slot);
/* c[(t A + a) 64 W + s] = sum_x s_x(now) s_x(snapshot in `slot`).  TSU_E_INVALID for a slot never taken.  Synchronous. */
int tsu_msc_snapshot_overlap(tsu_msc* h, int slot, int64_t* c);
/* A quench: times[0 .. n_times) are strictly ascending sweep counts since the start of the call, times[0] >= 0 (0: before the
 * first sweep).  For each k it enqueues times[k] - times[k - 1] sweeps by the handle's route (sweep counter sweep0 + times[k - 1]),
 * one measurement row, one C4 row, if k == wait_index[j] (ascending, n_wait <= the handle's snapshot slots) a snapshot into slot j,
 * and for every j whose snapshot this run has taken, this one included, one row of two-time correlations.  Nothing synchronises
 * with the host.  The planes at the end are those of tsu_msc_sweep(h, times[n_times - 1], sweep0) bit for bit, and
 * tsu_msc_launch_count advances by what that call adds (the small route starts one launch per span of sweeps here; the count
 * still advances by that call's one).  Needs a periodic axis, as tsu_msc_c4 does. */
int tsu_msc_quench_run(tsu_msc* h, int n_times, const int* times, uint32_t sweep0, int n_wait, const int* wait_index);
/* The rows of the last quench run (n_times must be its count): unsat, sum, q, q_link [n_times] x tsu_msc_measure's layouts and
 * conversions (q, q_link may be NULL; with one replica they are not written), c_z, c_r, c_c [n_times] x tsu_msc_c4's layouts
 * (NULL exactly for the open axes), two_time [n_wait][n_times][n_temps A][64 W] (may be NULL when n_wait is 0), entries with k
 * before the snapshot 0.  Synchronous. */
int tsu_msc_quench_history(tsu_msc* h, int n_times, int64_t* unsat, int64_t* sum, int64_t* q, int64_t* q_link, int64_t* c_z,
                           int64_t* c_r, int64_t* c_c, int64_t* two_time);

#endif /* TSU_HIP_MULTISPIN_QUENCH_H */
