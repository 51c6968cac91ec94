/* tsu_hip_multispin_pt.h -- K9: parallel tempering of a multispin-coded glass, the swaps on the device (csrc/multispin_pt.hip).
 *
 * Part of the C ABI of libtsu_hip.so: included by tsu_hip.h after tsu_hip_multispin.h (inside its extern "C" block); include
 * tsu_hip.h, not this file.  Its ctypes prototypes are tsu._hip.MULTISPIN_PT_SIGNATURES, one to one.
 *
 * Contract ("Tempering of multispin-coded glasses (K9)").  The functions take a tsu_msc handle with its
 * couplings, seeds and temperatures set.  A round is, in order: swap_interval sweeps of every plane (tsu_msc_sweep's, the shared
 * sweep counter); one measurement of every plane (tsu_msc_measure's integers, left on the device); one swap pass; the exchange.
 * The pass runs per sample s (the valid bits) and per replica a, independently, over the pairs i = 0 .. n_temps - 2 in order:
 * with E_x the energy (2 unsat - N_b, a double) of the configuration now at slot i and E_y that at slot i + 1,
 * delta = (1.0 / T[i] - 1.0 / T[i + 1]) * (E_x - E_y), accept iff delta >= 0 || u < exp(delta) in float64,
 * u = dense_uniform(i, round, TSU_TAG_PT_SWAP | a << 8) under the key swap_seeds[s].  An accepted pair exchanges the two
 * configurations of that sample, d = (x ^ y) & m per word; temperature, threshold table and sweep seed stay with the slot.  Pad
 * bits never swap.  Per (replica, sample): attempts and accepts per pair, which starting configuration (label) sits at which slot,
 * and flags and round trips per label by the ladders' rule (a label reaching slot 0 is BOTTOM, the one starting there included; a
 * BOTTOM label reaching the last slot is TOP; a TOP label reaching slot 0 counts one trip).
 */
#ifndef TSU_HIP_MULTISPIN_PT_H
#define TSU_HIP_MULTISPIN_PT_H
#ifndef TSU_HIP_H
#error "include tsu_hip.h, which includes this header"
#endif

/* Allocates (or resets) the tempering state of the handle: labels in starting order, counters 0.  T[n_temps]: the temperatures
 * given to tsu_msc_set_temperatures, which the swap pass needs as doubles.  TSU_E_INVALID unless 2 <= n_temps <= 256. */
int tsu_msc_pt_enable(tsu_msc* h, const double* T);
/* swap_seeds[n_samples]: the Philox key of sample s's swap uniforms, the same for both replicas (the replica is in the tag) */
int tsu_msc_pt_set_swap_seeds(tsu_msc* h, const uint64_t* swap_seeds);
/* n_rounds rounds, the first with sweep counter sweep0 and round counter round0.  do_swap = 0: no pass, no exchange.  record != 0:
 * every round's measurement is kept as a row on the device (taken after the round's sweeps, before its pass), replacing the rows of
 * the run before.  swap_interval = 0 is allowed: rounds without sweeps, a measurement and a pass each.  Asynchronous: nothing comes
 * back to the host. */
int tsu_msc_pt_run(tsu_msc* h, int n_rounds, int swap_interval, int do_swap, int record, uint32_t sweep0, uint32_t round0);
/* attempts, accepts: [replicas][n_samples][n_temps - 1]; labels (which starting configuration sits at the slot), flags and trips
 * (per label; flags 0 none, 1 BOTTOM, 2 TOP): [replicas][n_samples][n_temps].  Synchronous. */
int tsu_msc_pt_stats(tsu_msc* h, int64_t* attempts, int64_t* accepts, int32_t* labels, int32_t* flags, int64_t* trips);
/* The n_rows rounds recorded by the last run (n_rows must be that number), every row in tsu_msc_measure's layout with W * 64
 * columns: unsat, sum [n_rows][n_temps][replicas][64 W]; with two replicas q, q_link [n_rows][n_temps][64 W] (NULL allowed).
 * Synchronous. */
int tsu_msc_pt_history(tsu_msc* h, int n_rows, int64_t* unsat, int64_t* sum, int64_t* q, int64_t* q_link);
/* launches of the measurement, plan and exchange kernels by tsu_msc_pt_run so far (tsu_msc_launch_count: the sweeps') */
int tsu_msc_pt_launch_count(tsu_msc* h, uint64_t* out);

#endif /* TSU_HIP_MULTISPIN_PT_H */
