/* tsu_hip_ensemble.h -- tempering ensembles: the ladders of many disorder samples of one lattice shape in one handle, 2-D (K7) and
 * 3-D (K8), every kernel of a round covering all samples in one launch (csrc/pte_host.h, csrc/pt_host.h, entry points in
 * csrc/ising2d_disorder.hip and csrc/ising3d.hip).
 *
 * Part of the C ABI of libtsu_hip.so: included by tsu_hip.h after tsu_hip_overlap.h (inside its extern "C" block); include
 * tsu_hip.h, not this file.  Its ctypes prototypes are tsu._hip.ENSEMBLE_SIGNATURES, one to one.
 */
#ifndef TSU_HIP_ENSEMBLE_H
#define TSU_HIP_ENSEMBLE_H
#ifndef TSU_HIP_H
#error "include tsu_hip.h, which includes this header"
#endif

/* ------------------------------------------------------------------ K7 / K8: tempering ensembles over disorder samples
 * S samples x n_ladders (1 or 2) ladders x R temperatures (2 .. 256) of one lattice shape (any shape the lattice's create takes,
 * with its validation and messages) and ONE temperature table.  Walker g = (s n_ladders + k) R + w is walker w of ladder k of
 * sample s: Philox key seeds[s] + k R + w, replica 0, the handle's shared sweep counter, start slot w.  The swap uniforms of
 * sample s: key seeds[s], tag TAG_PT_SWAP | k << 8, counter = the round counter.  So sample s is tsu_pt2d / tsu_pt3d on disorder s
 * with seed = seeds[s], bit for bit: spins, E, M, q, walker, L, modes, attempts, accepts, round trips, slot tables, counters; with
 * swaps on or off, for split runs, and for every walker group the sweeps use (TSU_PT_GROUP; a group never straddles two samples).
 *
 * A round is the ladders' round with the sample as one more grid index: one launch per half-sweep, one energy partial pass, one
 * final pass, one swap pass (a wave per sample and ladder) and, if it records, one pass each for q, L, the profiles and the modes,
 * for all samples; the host waits for nothing.  Limits (refused before anything is allocated): S >= 1, S n_ladders R <= 65535 (the
 * energy pass's grid; it also bounds the sweep's S ceil(n_ladders R / W) groups).  Memory: all spin planes in one allocation, the
 * disorder in one allocation [S][J_right, J_down, (J_layer,) h][plane], 16 KiB of energy partials per walker.  No cluster moves.
 *
 * Call order: create, set_disorder, set_temperatures, init, then run and the readers (TSU_E_INVALID with a message naming the
 * missing call otherwise).  Array layouts are the ladders' with a leading sample axis. */
typedef struct tsu_pte2d tsu_pte2d;
typedef struct tsu_pte3d tsu_pte3d;
int tsu_pte2d_create(tsu_ctx* ctx, int rows, int cols, int periodic, int n_samples, int n_temps, int n_ladders, tsu_pte2d** out);
int tsu_pte3d_create(tsu_ctx* ctx, int depth, int rows, int cols, int periodic_mask, int n_samples, int n_temps, int n_ladders,
                     tsu_pte3d** out);
int tsu_pte2d_destroy(tsu_pte2d* pt);
int tsu_pte3d_destroy(tsu_pte3d* pt);
/* [S][lattice shape] arrays; each sample's arrays pass the lattice's set_disorder (its validation and messages).  Synchronises. */
int tsu_pte2d_set_disorder(tsu_pte2d* pt, const float* J_right, const float* J_down, const float* h /*nullable*/);
int tsu_pte3d_set_disorder(tsu_pte3d* pt, const float* J_right, const float* J_down, const float* J_layer, const float* h /*nullable*/);
int tsu_pte2d_set_temperatures(tsu_pte2d* pt, const double* T);
int tsu_pte3d_set_temperatures(tsu_pte3d* pt, const double* T);
/* seeds[S]; initial 0: random (walker g's draw is the lattice's randomize with its key), +1 / -1: all up / down; one launch for all */
int tsu_pte2d_init(tsu_pte2d* pt, const uint64_t* seeds, int initial);
int tsu_pte3d_init(tsu_pte3d* pt, const uint64_t* seeds, int initial);
int tsu_pte2d_run(tsu_pte2d* pt, int n_rounds, int swap_interval, int do_swap, int record);
int tsu_pte3d_run(tsu_pte3d* pt, int n_rounds, int swap_interval, int do_swap, int record);
/* the last run's rows: E, M, walker [round][sample][ladder][slot]; q [round][sample][slot] (two ladders).  Synchronises. */
int tsu_pte2d_history(tsu_pte2d* pt, double* E, int64_t* M, int64_t* q, int32_t* walker);
int tsu_pte3d_history(tsu_pte3d* pt, double* E, int64_t* M, int64_t* q, int32_t* walker);
/* attempts, accepts [sample][ladder][R - 1]; round_trips, walker_at_slot [sample][ladder][R]; any pointer may be NULL */
int tsu_pte2d_stats(tsu_pte2d* pt, int64_t* attempts, int64_t* accepts, int64_t* round_trips, int32_t* walker_at_slot,
                    uint64_t* sweep_count, uint64_t* round_count);
int tsu_pte3d_stats(tsu_pte3d* pt, int64_t* attempts, int64_t* accepts, int64_t* round_trips, int32_t* walker_at_slot,
                    uint64_t* sweep_count, uint64_t* round_count);
/* every walker's E and sum of spins now, [sample][ladder][walker].  Synchronises. */
int tsu_pte2d_energies(tsu_pte2d* pt, double* E, int64_t* sum_s);
int tsu_pte3d_energies(tsu_pte3d* pt, double* E, int64_t* sum_s);
/* the spins of the walker now at (sample, ladder, slot), int8 row-major in the lattice's shape.  Synchronises. */
int tsu_pte2d_get_spins(tsu_pte2d* pt, int sample, int ladder, int slot, int8_t* host);
int tsu_pte3d_get_spins(tsu_pte3d* pt, int sample, int ladder, int slot, int8_t* host);
int tsu_pte2d_set_spins(tsu_pte2d* pt, int sample, int ladder, int slot, const int8_t* host);
int tsu_pte3d_set_spins(tsu_pte3d* pt, int sample, int ladder, int slot, const int8_t* host);
/* half-sweep launches so far (one per half-sweep for all walkers of all samples) */
int tsu_pte2d_launch_count(tsu_pte2d* pt, uint64_t* n_launches);
int tsu_pte3d_launch_count(tsu_pte3d* pt, uint64_t* n_launches);
/* as the ladders' (tsu_hip_correlation.h): modes [round][sample][slot][periodic axis][re, im] */
int tsu_pte2d_set_correlation(tsu_pte2d* pt, int enable, const double* cos_row, const double* sin_row, const double* cos_col,
                              const double* sin_col);
int tsu_pte3d_set_correlation(tsu_pte3d* pt, int enable, const double* cos_z, const double* sin_z, const double* cos_r,
                              const double* sin_r, const double* cos_c, const double* sin_c);
int tsu_pte2d_history_modes(tsu_pte2d* pt, double* modes);
int tsu_pte3d_history_modes(tsu_pte3d* pt, double* modes);
/* as the ladders' (tsu_hip_overlap.h): L [round][sample][slot], two ladders only */
int tsu_pte2d_set_link_overlap(tsu_pte2d* pt, int enable);
int tsu_pte3d_set_link_overlap(tsu_pte3d* pt, int enable);
int tsu_pte2d_history_link(tsu_pte2d* pt, int64_t* L);
int tsu_pte3d_history_link(tsu_pte3d* pt, int64_t* L);
/* the axis profiles of the walkers now at (sample, slot): of the spins, or with two ladders of the product of the two.  Synchronises. */
int tsu_pte2d_profiles(tsu_pte2d* pt, int sample, int slot, int64_t* p_row, int64_t* p_col);
int tsu_pte3d_profiles(tsu_pte3d* pt, int sample, int slot, int64_t* p_z, int64_t* p_r, int64_t* p_c);

#endif /* TSU_HIP_ENSEMBLE_H */
