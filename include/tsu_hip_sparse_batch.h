/* tsu_hip_sparse_batch.h -- K5 walker batches: n_ladders ladders of n_temps walkers on the CSR graph of ONE tsu_sparse handle, with
 * batched half-sweeps, fixed-order energies and the swap pass of the lattice ladders (csrc/sparse_batch.hip,
 * csrc/sparse_batch_dev.h).
 *
 * Part of the C ABI of libtsu_hip.so: included by tsu_hip.h after tsu_hip_ensemble.h (inside its extern "C" block); include
 * tsu_hip.h, not this file.  Its ctypes prototypes are tsu._hip.SPARSE_BATCH_SIGNATURES, one to one.
 */
#ifndef TSU_HIP_SPARSE_BATCH_H
#define TSU_HIP_SPARSE_BATCH_H
#ifndef TSU_HIP_H
#error "include tsu_hip.h, which includes this header"
#endif

/* ------------------------------------------------------------------ K5: tempering and annealing of a sparse graph, many walkers
 * Walker g = ladder n_temps + w starts at slot w; all walkers share one sweep counter (0 after init).  A sweep of walker g is
 * tsu_sparse_sweep(graph, T of its slot, 1, seed, sweep, replica = g) bit for bit (the generic K5 expression for every colour class);
 * the random start is bit i = [uniform53(i, 0, TAG_INIT | g << 8, seed) < 0.5]; the swap pass is the lattice ladders' (tag
 * TAG_PT_SWAP | ladder << 8, key = seed, counter = the round; detailed-balance rule).  The energy of a walker is a FIXED-ORDER double
 * sum, the same bits on every run and on both routes: per position p the term -0.5 b F - bias b with F summed in CSR order; per
 * segment of 65536 positions the 1024 strided partials P_j (p = j mod 1024, ascending), reduced by the halving tree P_j += P_{j+s},
 * s = 512 .. 1; the segments' sums added in ascending order.  ("Walker batches on a sparse graph".)
 *
 * Two routes, chosen per call: the COLOUR route (any n: one launch per colour class for all walkers, state[position][walker]) and
 * the SMALL route (n <= 32768: one workgroup per walker, the state in LDS, all sweeps of a round and the energy in one launch).
 * TSU_K5B_SMALL=0 forces the colour route.  Nothing in run waits for the device.
 *
 * Limits (refused before anything is allocated): 1 <= n_temps <= 256, n_ladders >= 1, n_temps n_ladders <= 65535.  The batch borrows
 * the graph: it must outlive the batch, and its own resident state is not touched.
 * Call order: create, set_temperatures, init, then run and the readers. */
typedef struct tsu_sparse_batch tsu_sparse_batch;
int tsu_sparse_batch_create(tsu_sparse* graph, int n_temps, int n_ladders, tsu_sparse_batch** out);
int tsu_sparse_batch_destroy(tsu_sparse_batch* b);
/* T[n_temps], slot -> temperature, all > 0; enqueued on the stream (no wait), may be called between runs */
int tsu_sparse_batch_set_temperatures(tsu_sparse_batch* b, const double* T);
/* initial 0: random (above), 1: all bits one, -1: all bits zero; resets the tables, the counters and the best states.  Synchronises. */
int tsu_sparse_batch_init(tsu_sparse_batch* b, uint64_t seed, int initial);
/* the bits {0,1} of the walker now at (ladder, slot), site order, n bytes.  Synchronise. */
int tsu_sparse_batch_set_state(tsu_sparse_batch* b, int ladder, int slot, const int8_t* bits_host);
int tsu_sparse_batch_get_state(tsu_sparse_batch* b, int ladder, int slot, int8_t* bits_host);
/* n_rounds rounds of swap_interval sweeps of every walker, then (do_swap or record or best tracking) the energies, (best tracking)
 * the best-state passes, (do_swap or record) the swap pass, which also writes the round's history row when record is set */
int tsu_sparse_batch_run(tsu_sparse_batch* b, int n_rounds, int swap_interval, int do_swap, int record);
/* the last recording run's rows [round][ladder][slot]: E, sum of spins, walker.  Any pointer may be NULL.  Synchronises. */
int tsu_sparse_batch_history(tsu_sparse_batch* b, double* E, int64_t* M, int32_t* walker);
/* attempts, accepts [ladder][n_temps - 1]; round_trips, walker_at_slot [ladder][n_temps]; any pointer may be NULL.  Synchronises. */
int tsu_sparse_batch_stats(tsu_sparse_batch* b, int64_t* attempts, int64_t* accepts, int64_t* round_trips, int32_t* walker_at_slot,
                           uint64_t* sweep_count);
/* every walker's energy and sum of spins now, [ladder][walker].  Synchronises. */
int tsu_sparse_batch_energies(tsu_sparse_batch* b, double* E, int64_t* sum_s);
/* best-state tracking (off after create): after each energy pass of a run every walker keeps its lowest-energy state so far and that
 * energy (strict <: the first minimum stays); the state a run starts from is a candidate.  Off: a run's launches are what they were. */
int tsu_sparse_batch_track_best(tsu_sparse_batch* b, int enable);
/* the lowest best energy among the walkers of `ladder` (the first such walker), its bits (site order, nullable) and the walker */
int tsu_sparse_batch_best(tsu_sparse_batch* b, int ladder, double* E, int8_t* bits_host /*nullable*/, int32_t* walker);
/* six int32: route of the next run (0 colour, 1 small), walkers per thread, padded walkers, launches per sweep, further launches of
 * a round that swaps or records (energy passes + swap pass; + 2 with best tracking), energy segments */
#define TSU_SPARSE_BATCH_PLAN_LEN 6
int tsu_sparse_batch_plan(tsu_sparse_batch* b, int32_t* rec /*6*/);
/* kernel launches enqueued by run so far (every kind) */
int tsu_sparse_batch_launch_count(tsu_sparse_batch* b, uint64_t* n_launches);

#endif /* TSU_HIP_SPARSE_BATCH_H */
