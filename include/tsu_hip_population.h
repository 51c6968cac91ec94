/* tsu_hip_population.h -- population annealing of disordered lattices, 2-D (K7) and 3-D (K8), with the resampling on the device
 * (csrc/pop_dev.h, csrc/pop_host.h, entry points in csrc/ising2d_disorder.hip and csrc/ising3d.hip).
 *
 * Part of the C ABI of libtsu_hip.so: included by tsu_hip.h after tsu_hip_correlation.h (inside its extern "C" block); include
 * tsu_hip.h, not this file.  Its ctypes prototypes are tsu._hip.POPULATION_SIGNATURES, one to one.
 */
#ifndef TSU_HIP_POPULATION_H
#define TSU_HIP_POPULATION_H
#ifndef TSU_HIP_H
#error "include tsu_hip.h, which includes this header"
#endif

/* ------------------------------------------------------------------ K7 / K8: population annealing on one disorder
 * A population of R walkers (2 .. 65535, fixed), every walker a whole K7 / K8 lattice (any shape the lattice's create takes, with
 * its validation and messages), all sharing ONE disorder, annealed along beta[0] < beta[1] < .. < beta[K], beta[0] >= 0.  Walker i
 * has Philox key seed + i, replica 0, the handle's shared sweep counter and the initial draw of the lattice's randomize with
 * (seed + i, 0): it is a ladder's walker.  The key belongs to the index i, not to the configuration, so copies diverge.
 *
 * init: the draw; if beta[0] > 0, initial_sweeps sweeps at 1 / beta[0]; one energy pass (E_i, sum of spins M_i: the ladders' bits).
 * Step k = 1 .. K, db = beta[k] - beta[k - 1], in float64 then integers only:
 *   E_min = min_i E_i;  W_i = (uint32) rint(exp(-(db (E_i - E_min))) 2^30);  S = sum_i W_i;
 *   U = mulhi64(x64, S), x64 = (w1 << 32) | w0 of Philox(0, 0, k_abs, tag 11 (TAG_POP_RESAMPLE)), key = seed, k_abs = the number of
 *   steps taken since init before this one;
 *   n_i = (R C_i + U) / S - (R C_{i-1} + U) / S, C_i the inclusive prefix sums of W, C_{-1} = 0: sum n_i = R, n_i = floor or ceil of
 *   R W_i / S (weights below 2^-31 of the largest count as 0);
 *   a walker with n_i >= 1 stays (parent[i] = i); the dead indices, ascending, take the extra copies in ascending order of their
 *   source (source g: n_g - 1 times); the planes parent[i] -> i of the dead i are copied;
 *   sweeps_per_step sweeps of every walker at T = 1 / beta[k] (one launch per half-sweep for all walkers), one energy pass: the
 *   record's row and the next step's E_i.
 * resample = 0 skips the weights, the plan and the copy: walker i is then the single lattice with seed + i swept at each 1 / beta[k]
 * bit for bit.  Within run the host waits for nothing.  DESIGN.md section 3, "Population annealing".
 *
 * Call order: create, set_disorder, set_schedule, init, then run, energies, get_spins, set_spins (TSU_E_INVALID with a message
 * naming the missing call otherwise).
 * set_schedule after init asks for a new init.  An allocation that does not fit returns TSU_E_NOMEM and leaves nothing behind. */
typedef struct tsu_pa2d tsu_pa2d;
typedef struct tsu_pa3d tsu_pa3d;
int tsu_pa2d_create(tsu_ctx* ctx, int rows, int cols, int periodic, int population, tsu_pa2d** out);
int tsu_pa3d_create(tsu_ctx* ctx, int depth, int rows, int cols, int periodic_mask, int population, tsu_pa3d** out);
int tsu_pa2d_destroy(tsu_pa2d* pa);
int tsu_pa3d_destroy(tsu_pa3d* pa);
/* the same arrays, validation and messages as the lattice's set_disorder; stored once for all walkers */
int tsu_pa2d_set_disorder(tsu_pa2d* pa, const float* J_right, const float* J_down, const float* h /*nullable*/);
int tsu_pa3d_set_disorder(tsu_pa3d* pa, const float* J_right, const float* J_down, const float* J_layer, const float* h /*nullable*/);
/* n >= 2 inverse temperatures, increasing, betas[0] >= 0: n - 1 steps.  Synchronises. */
int tsu_pa2d_set_schedule(tsu_pa2d* pa, const double* betas, int n);
int tsu_pa3d_set_schedule(tsu_pa3d* pa, const double* betas, int n);
int tsu_pa2d_init(tsu_pa2d* pa, uint64_t seed, int initial_sweeps);
int tsu_pa3d_init(tsu_pa3d* pa, uint64_t seed, int initial_sweeps);
/* n_steps further steps from the handle's step counter; running past the schedule: TSU_E_INVALID.  Asynchronous. */
int tsu_pa2d_run(tsu_pa2d* pa, int n_steps, int sweeps_per_step, int resample, int record);
int tsu_pa3d_run(tsu_pa3d* pa, int n_steps, int sweeps_per_step, int resample, int record);
/* The rows of the last run, which must have recorded (n = its n_steps; any pointer may be NULL): E, M [n + 1][R], row 0 the
 * population the run started from, row j the one after its step j; W, parent [n][R]; S, U, E_min [n].  A run with resample = 0
 * records parent = identity and W, S, U, E_min = 0.  Synchronises. */
int tsu_pa2d_history(tsu_pa2d* pa, double* E, int64_t* M, uint32_t* W, int32_t* parent, uint64_t* S, uint64_t* U, double* E_min);
int tsu_pa3d_history(tsu_pa3d* pa, double* E, int64_t* M, uint32_t* W, int32_t* parent, uint64_t* S, uint64_t* U, double* E_min);
/* every walker's E and sum of spins now, by walker.  Synchronises. */
int tsu_pa2d_energies(tsu_pa2d* pa, double* E, int64_t* sum_s);
int tsu_pa3d_energies(tsu_pa3d* pa, double* E, int64_t* sum_s);
/* walker i's spins, int8 row-major in the lattice's shape.  Synchronises. */
int tsu_pa2d_get_spins(tsu_pa2d* pa, int i, int8_t* host);
int tsu_pa3d_get_spins(tsu_pa3d* pa, int i, int8_t* host);
int tsu_pa2d_set_spins(tsu_pa2d* pa, int i, const int8_t* host);
int tsu_pa3d_set_spins(tsu_pa3d* pa, int i, const int8_t* host);
/* half-sweep launches so far (one per half-sweep for all walkers) */
int tsu_pa2d_launch_count(tsu_pa2d* pa, uint64_t* n_launches);
int tsu_pa3d_launch_count(tsu_pa3d* pa, uint64_t* n_launches);

#endif /* TSU_HIP_POPULATION_H */
