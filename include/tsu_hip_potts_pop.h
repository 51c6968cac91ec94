/* tsu_hip_potts_pop.h -- K14: population annealing of K12's Potts lattice with per-bond couplings and per-site colour fields, in 2-D
 * and 3-D, the resampling on the GPU (csrc/potts_pop.hip, potts_pop_kern_dev.h, potts_pop_plan.h; the resampling kernels are
 * pop_dev.h's).  The counterpart of tsu_pa2d_* / tsu_pa3d_* for Potts glasses, random-bond and diluted Potts models and the Potts
 * prior with unary costs: the one method here that yields ln Z, F and the entropy of such a model.
 *
 * Part of the C ABI of libtsu_hip.so: included by tsu_hip.h (inside its extern "C" block, after tsu_hip_potts_pt.h, whose lattice,
 * disorder layout, heat-bath rule and measuring order it shares); include tsu_hip.h, not this file.  Its ctypes prototypes are
 * tsu._hip.POTTS_POP_SIGNATURES, one to one.
 *
 * Contract ("Population annealing of Potts lattices (K14)"; tests/helpers/potts_pop_twin.py is its NumPy twin):
 * a population of R walkers (2 .. 65535, fixed) on ONE K12 disorder, annealed along beta[0] < .. < beta[K], beta[0] >= 0.  Walker i
 * is a whole K12 lattice with Philox key seed + i (mod 2^64), replica 0 and the handle's shared 32-bit sweep counter.  The key
 * belongs to the index i, not to the colours, so copies diverge.  The walkers sit in one allocation at a stride of `sites` rounded
 * up to a multiple of 16 bytes; the pad bytes are zero and no sweep or measuring pass reads them.
 *
 * init(seed, initial, initial_sweeps): initial in 0 .. q - 1 puts that colour everywhere; -1 keeps the colours as they are (for
 * set_spins); -2 draws on the device: site (rho, c) of walker i, rho = z rows + r, gets ((uint64) W q) >> 32 with W = word c & 3 of
 * Philox(c >> 2, rho, 0, TAG_INIT), key seed + i (uniform to within q 2^-32; the rule of the cluster colours; no new stream tag).
 * Then, if beta[0] > 0, initial_sweeps sweeps at 1 / beta[0]; then one measuring pass.
 * Step k = 1 .. K, db = beta[k] - beta[k - 1], exactly the step of tsu_hip_population.h, in float64 then integers only:
 *   E_min = min_i E_i;  W_i = (uint32) rint(exp(-(db (E_i - E_min))) 2^30);  S = sum_i W_i;
 *   U = mulhi64(x64, S), x64 = (w1 << 32) | w0 of Philox(0, 0, k_abs, TAG_POP_RESAMPLE), key = seed, k_abs = the steps taken since
 *   init before this one;  n_i = (R C_i + U) / S - (R C_{i-1} + U) / S with the inclusive prefix sums C_i of W: sum n_i = R;
 *   a walker with n_i >= 1 stays (parent[i] = i); the dead indices, ascending, take the extra copies in ascending order of their
 *   source; the planes parent[i] -> i of the dead i are copied;
 *   sweeps_per_step K12 heat-bath sweeps of every walker at the double T = 1.0 / beta[k];
 *   one measuring pass: every walker's float64 E (the bits of tsu_potts_dis_measure on the same colours), n_eq and N_0 .. N_7: the
 *   record's row and the next step's E_i.
 * resample = 0 skips the plan and the copy: walker i is then tsu_potts_dis_sweep(1 / beta[k], .., seed + i, sweep counter, 0) on the
 * same colours, bit for bit.  Within run the host waits for nothing.  Results depend on (colours, q, disorder, schedule, seed,
 * counters) only, never on the route.
 *
 * Call order: create, set_disorder, set_schedule, init, then run and energies (TSU_E_INVALID with a message naming the missing call
 * otherwise); get_spins and set_spins at any time after create.  set_schedule after init asks for a new init. */
#ifndef TSU_HIP_POTTS_POP_H
#define TSU_HIP_POTTS_POP_H
#ifndef TSU_HIP_H
#error "include tsu_hip.h, which includes this header"
#endif

typedef struct tsu_potts_pop tsu_potts_pop;

#define TSU_POTTS_POP_ROUTE_PACK 0  /* k14_pop_pack: G >= 2 walkers a workgroup, colours and the disorder in LDS, one launch a step */
#define TSU_POTTS_POP_ROUTE_SMALL 1 /* k14_pop_small: at most 16384 sites, one workgroup per walker, one launch a step */
#define TSU_POTTS_POP_ROUTE_SWEEP 2 /* k14_pop_sweep: one launch per half-sweep for all walkers through HBM */

/* `population` walkers of a depth x rows x cols lattice of q colours; periodic: three flags (pz, pr, pc); depth 1 with an open z axis
 * is the 2-D lattice.  Refused before anything is allocated: tsu_potts_dis_create's shape checks (q outside 2 .. 8, an extent < 1,
 * 2^31 sites or more, a periodic axis of odd length) and a population outside 2 .. 65535.  A population that does not fit returns
 * TSU_E_NOMEM and leaves nothing behind.  The colours start as 0. */
int tsu_potts_pop_create(tsu_ctx* ctx, int depth, int rows, int cols, int q, const int* periodic, int population, tsu_potts_pop** out);
int tsu_potts_pop_destroy(tsu_potts_pop* pa);

/* the arrays, checks and messages of tsu_potts_dis_set_disorder; stored once for all walkers (synchronous) */
int tsu_potts_pop_set_disorder(tsu_potts_pop* pa, const float* J_right, const float* J_down, const float* J_layer, const float* h);
/* n >= 2 inverse temperatures, increasing, betas[0] >= 0: n - 1 steps.  The population has to be initialised again afterwards. */
int tsu_potts_pop_set_schedule(tsu_potts_pop* pa, const double* betas, int n);
/* see above; the sweep and step counters and what advance added return to 0, and the record is dropped */
int tsu_potts_pop_init(tsu_potts_pop* pa, uint64_t seed, int initial, int initial_sweeps);
/* moves the shared sweep counter on by n_sweeps without sweeping (the counter's words are 32-bit and wrap, as K12's) */
int tsu_potts_pop_advance(tsu_potts_pop* pa, uint64_t n_sweeps);

/* n_steps further steps from the handle's step counter, all enqueued.  Running past the schedule, or more than 2^31 sweeps since
 * init: TSU_E_INVALID.  Launches per step: on _PACK and _SMALL 1 (the sweeps; none when sweeps_per_step = 0) + 2 (measure, final
 * sums) + 2 when it resamples (plan, copy); on _SWEEP 2 sweeps_per_step + 2 (+ 2).  init launches 1 when it draws, its sweeps in the
 * same way, and the 2 of a measuring pass; energies launches 2; a run that records without resampling 1 more (the identity parent
 * rows).  TSU_POTTS_SMALL=0 in the environment (tests, read per call) sends
 * every lattice to _SWEEP; TSU_POTTS_POP_PACK=0 (tests, read per call) turns _PACK into _SMALL. */
int tsu_potts_pop_run(tsu_potts_pop* pa, int n_steps, int sweeps_per_step, int resample, int record);
/* The rows of the last run, which must have recorded (n = its n_steps; any pointer may be NULL): E, n_eq [n + 1][R] and N
 * [n + 1][R][8], row 0 the population the run started from, row j the one after its step j; W, parent [n][R]; S, U, E_min [n].  A
 * run with resample = 0 records parent = identity and W, S, U, E_min = 0.  Synchronises. */
int tsu_potts_pop_history(tsu_potts_pop* pa, double* E, int64_t* n_eq, int64_t* N, uint32_t* W, int32_t* parent, uint64_t* S, uint64_t* U,
                          double* E_min);
/* every walker's E and n_eq now, by walker (synchronises); E has the bits of tsu_potts_dis_measure */
int tsu_potts_pop_energies(tsu_potts_pop* pa, double* E, int64_t* n_eq);
/* walker i's colours: depth * rows * cols int8, row-major, every value in 0 .. q - 1.  Synchronises. */
int tsu_potts_pop_get_spins(tsu_potts_pop* pa, int i, int8_t* colours);
int tsu_potts_pop_set_spins(tsu_potts_pop* pa, int i, const int8_t* colours);
/* walker i's whole slot of the allocation: the colours followed by the pad, `sites` rounded up to a multiple of 16 bytes in all (the
 * pad bytes are 0 at all times; tests).  Synchronises. */
int tsu_potts_pop_get_padded(tsu_potts_pop* pa, int i, int8_t* bytes);
/* TSU_POTTS_POP_ROUTE_* a run would take now */
int tsu_potts_pop_route(tsu_potts_pop* pa, int* route);
/* what the packing rule (csrc/potts_pop_plan.h) gives this handle now: the route, the walkers of a workgroup (1 off _PACK), the
 * lanes of a sweep workgroup and its LDS bytes; any pointer may be NULL */
int tsu_potts_pop_plan(tsu_potts_pop* pa, int* route, int* G, int* threads, int* lds_bytes);
/* kernel launches of this handle so far */
int tsu_potts_pop_launch_count(tsu_potts_pop* pa, uint64_t* n);

#endif /* TSU_HIP_POTTS_POP_H */
