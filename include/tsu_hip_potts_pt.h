/* tsu_hip_potts_pt.h -- K13: parallel tempering (replica exchange) of K12's Potts lattice with per-bond couplings and per-site colour
 * fields, in 2-D and 3-D, the swaps on the GPU (csrc/potts_pt.hip, potts_pt_kern_dev.h).  The counterpart of tsu_pt2d_* / tsu_pt3d_*
 * for Potts glasses, random-bond and diluted Potts models and the Potts prior with unary costs.
 *
 * Part of the C ABI of libtsu_hip.so: included by tsu_hip.h (inside its extern "C" block, after tsu_hip_potts_disorder.h, whose
 * lattice, disorder layout and heat-bath rule it shares); include tsu_hip.h, not this file.  Its ctypes prototypes are
 * tsu._hip.POTTS_PT_SIGNATURES, one to one.
 *
 * Contract ("Parallel tempering (K13)"; tests/helpers/potts_pt_twin.py is its NumPy twin): n_ladders (1 or 2)
 * ladders of n_temps (2 .. 256) walkers on ONE disorder.  Walker g = k n_temps + w of ladder k is a whole K12 lattice with Philox key
 * seed + g (mod 2^64), replica 0 and the shared sweep counter; it starts at slot (temperature) w.  The key travels with the walker,
 * the temperature belongs to the slot: without swaps walker g is tsu_potts_dis_sweep(T[w], .., seed + g, sweep counter, 0) on the
 * same colours, bit for bit.  A round = swap_interval K12 heat-bath sweeps of every walker at its slot's temperature, then every
 * walker's n_eq, N_c and float64 E (the bits of tsu_potts_dis_measure on the same colours), then per ladder one swap pass: for
 * i = 0 .. n_temps - 2 in order, a / b = the walkers at slots i / i + 1, delta = (1 / T_i - 1 / T_{i+1}) (E_a - E_b) in float64,
 * accept iff delta >= 0 or u < exp(delta), u = the 53-bit uniform of Philox(i >> 1, 0, t, TSU_TAG_PT_SWAP | k << 8) with key seed
 * and t = the round counter (tsu_pt2d_run's pass, kernel and round-trip bookkeeping; no new stream tag); an accepted swap
 * exchanges the two walkers' slots, never their colours.  With two ladders the record of a round then holds, per slot, the exact
 * contingency table C[a][b] = the sites that show colour a in ladder 0's walker and colour b in ladder 1's walker at that slot
 * (sum = sites), from which the Potts overlap (q sum_a C[a][a] / sites - 1) / (q - 1) and the permutation-symmetric overlaps follow.
 * Results depend on (colours, q, disorder, temperatures, seed, counters) only, never on the route. */
#ifndef TSU_HIP_POTTS_PT_H
#define TSU_HIP_POTTS_PT_H
#ifndef TSU_HIP_H
#error "include tsu_hip.h, which includes this header"
#endif

typedef struct tsu_potts_pt tsu_potts_pt;

#define TSU_POTTS_PT_ROUTE_SMALL 0 /* k13_pt_small: at most 16384 sites, one workgroup per walker, a round's sweeps in one launch */
#define TSU_POTTS_PT_ROUTE_SWEEP 1 /* k13_pt_sweep: one launch per half-sweep for all walkers through HBM */

/* n_ladders ladders of n_temps walkers of a depth x rows x cols lattice of q colours; periodic: three flags (pz, pr, pc); depth 1
 * with an open z axis is the 2-D lattice.  Refused before anything is allocated: tsu_potts_dis_create's shape checks (q outside
 * 2 .. 8, an extent < 1, 2^31 sites or more, a periodic axis of odd length), n_temps outside 2 .. 256, n_ladders outside 1 .. 2.
 * All colours sit in one allocation, with one copy of the disorder; a ladder that does not fit returns TSU_E_NOMEM and leaves
 * nothing behind.  The colours start as 0, every walker at its own slot. */
int tsu_potts_pt_create(tsu_ctx* ctx, int depth, int rows, int cols, int q, const int* periodic, int n_temps, int n_ladders,
                        tsu_potts_pt** out);
int tsu_potts_pt_destroy(tsu_potts_pt* pt);

/* the arrays, checks and messages of tsu_potts_dis_set_disorder; stored once for all walkers (synchronous) */
int tsu_potts_pt_set_disorder(tsu_potts_pt* pt, const float* J_right, const float* J_down, const float* J_layer, const float* h);
/* T[slot], n_temps values, each finite and > 0 (TSU_E_INVALID otherwise, the stored ladder untouched) */
int tsu_potts_pt_set_temperatures(tsu_potts_pt* pt, const double* T);

/* the colours of the walker now at (ladder, slot): depth * rows * cols int8, row-major, every value in 0 .. q - 1 */
int tsu_potts_pt_set_spins(tsu_potts_pt* pt, int ladder, int slot, const int8_t* colours);
int tsu_potts_pt_get_spins(tsu_potts_pt* pt, int ladder, int slot, int8_t* colours);

/* Walker g gets the key seed + g; every walker returns to its own slot; counters, statistics and the record are reset.  initial in
 * 0 .. q - 1: that colour everywhere; initial = -1: the colours stay as they are, for a caller that sets them by
 * tsu_potts_pt_set_spins (tsu.PottsTempering draws default_rng(seed + g).integers(0, q, shape) on the host). */
int tsu_potts_pt_init(tsu_potts_pt* pt, uint64_t seed, int initial);
/* moves the shared sweep counter on by n_sweeps without sweeping (the counter's words are 32-bit and wrap, as K12's) */
int tsu_potts_pt_advance(tsu_potts_pt* pt, uint64_t n_sweeps);

/* n_rounds rounds, all enqueued: no host synchronisation.  do_swap = 0: no swap pass.  record: after each round's pass, per (ladder,
 * slot), E, n_eq, N_0 .. N_7 of the walker there and which walker it is, and with two ladders the table of every slot (the rows of
 * this run replace those of the previous one).  A round launches its sweeps (TSU_POTTS_PT_ROUTE_SMALL: 1; _SWEEP: 2 swap_interval)
 * plus, when it swaps or records, 3 (measure, final sums, swap pass), plus 1 when it records (the colour counts), plus 1 when it
 * records two ladders (the tables).  TSU_POTTS_SMALL=0 in the environment (tests, read per call) sends every lattice to k13_pt_sweep. */
int tsu_potts_pt_run(tsu_potts_pt* pt, int n_rounds, int swap_interval, int do_swap, int record);
/* the rows of the last run (synchronises): E, n_eq, walker [round][ladder][slot]; N [round][ladder][slot][8]; any may be NULL */
int tsu_potts_pt_history(tsu_potts_pt* pt, double* E, int64_t* n_eq, int64_t* N, int32_t* walker);
/* the tables of the last run, [round][slot][a][b] with a, b < q (q * q words a slot); two ladders only */
int tsu_potts_pt_overlap_tables(tsu_potts_pt* pt, int64_t* tables);
/* attempts, accepts [ladder][pair]; round_trips [ladder][walker]; walker_at_slot [ladder][slot]; any pointer may be NULL */
int tsu_potts_pt_stats(tsu_potts_pt* pt, int64_t* attempts, int64_t* accepts, int64_t* round_trips, int32_t* walker_at_slot,
                       uint64_t* sweep_count, uint64_t* round_count);
/* every walker's E and n_eq now, indexed [ladder][walker] (synchronises); E has the bits of tsu_potts_dis_measure */
int tsu_potts_pt_energies(tsu_potts_pt* pt, double* E, int64_t* n_eq);
/* TSU_POTTS_PT_ROUTE_* a run would take now */
int tsu_potts_pt_route(tsu_potts_pt* pt, int* route);
/* kernel launches of this handle so far */
int tsu_potts_pt_launch_count(tsu_potts_pt* pt, uint64_t* n);

#endif /* TSU_HIP_POTTS_PT_H */
