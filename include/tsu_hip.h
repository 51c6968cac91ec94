/*
 * tsu_hip.h -- C ABI of libtsu_hip.so: the MI355X (gfx950) stochastic spin-update hot path.
 *
 * The reference (Arsham-001/tsu-emulator) is pure Python/NumPy and has NO FFI: its boundary for this
 * path is the Python method surface of tsu/gibbs.py, tsu/models/ising.py and tsu/core.py.  This header
 * is the boundary a host-language binding would bind instead; every entry point names the reference
 * interface it replaces (file:line under /root/reference).  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++ / torch types.
 *   - every function returns int: TSU_OK or a negative TSU_E_*; tsu_last_error() gives the text.
 *     No exceptions or longjmp cross the ABI.
 *   - the caller owns all host buffers (never retained past the call); the library owns device
 *     memory behind opaque handles with explicit create/destroy.
 *   - handles are not thread-safe; one tsu_ctx per process per device.
 *   - all work is enqueued on the ctx stream (tsu_set_stream; default: the null stream).  Calls that
 *     copy results to host memory synchronise that stream before returning; pure device calls
 *     (sweep, step, randomize) are asynchronous.
 *   - randomness is counter-based Philox4x32-10 keyed by (seed, position, sweep/step counter): results
 *     do not depend on launch geometry, tile size, number of sweeps per call, or slab decomposition.
 *   - limits of the counters, the same at every entry point (TSU_E_INVALID beyond them, nothing launched, no state touched):
 *       replica ids (scalar or per-lattice / per-replica arrays) are below 2^24: the id shares a Philox counter word with the
 *         8-bit stream tag (TAG | replica << 8);
 *       lattice sweeps (K1, K7, K8: the half-sweep counter is 2 sweep + colour) take sweep0 + n_sweeps <= 2^31;
 *       cluster steps take step0 + n_steps <= 2^32; dense and sparse sweeps (K2, K5) take sweep0 + total sweeps <= 2^32;
 *       a counter never wraps to replay the stream of sweep 0.  Langevin chain ids and step counters are full 32-bit words.
 */
#ifndef TSU_HIP_H
#define TSU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSU_OK 0
#define TSU_E_INVALID (-1)     /* bad argument (Python side raises ValueError / ConfigurationError) */
#define TSU_E_NOMEM (-2)       /* host or device allocation failed */
#define TSU_E_HIP (-3)         /* a HIP runtime call failed */
#define TSU_E_RCCL (-4)        /* RCCL not loadable / a communicator call failed */
#define TSU_E_UNSUPPORTED (-5) /* valid request this build has no kernel for */

#define TSU_MODE_PHYSICAL 0 /* corrected spin->bit bias: P(+1) = sigmoid(2 (J nsum + h) / T) */
#define TSU_MODE_COMPAT 1   /* bias exactly as tsu/models/ising.py:148 (bug-for-bug) */

#define TSU_DTYPE_F64 0
#define TSU_DTYPE_F32 1

#define TSU_KERNEL_AUTO 0    /* pick the fastest kernel that supports the lattice */
#define TSU_KERNEL_GENERIC 1 /* one colour per launch, global memory, any shape / boundary */
#define TSU_KERNEL_TILED 2   /* LDS-staged halo tiles, several sweeps per launch */
#define TSU_KERNEL_SMALL 3   /* whole lattice of <= 1024 octets: resident in one workgroup's LDS, all sweeps in one launch
                                (one-row and one-column lattices: the generic kernel) */

typedef struct tsu_ctx tsu_ctx;
typedef struct tsu_ising2d tsu_ising2d;
typedef struct tsu_dense tsu_dense;
typedef struct tsu_langevin tsu_langevin;
typedef struct tsu_sparse tsu_sparse;
typedef struct tsu_comm tsu_comm;

/* ------------------------------------------------------------------ context */
int tsu_version(void);
/* device < 0: use the current HIP device.  Fails with TSU_E_HIP when no GPU is present. */
int tsu_init(int device, tsu_ctx** ctx);
int tsu_shutdown(tsu_ctx* ctx);
/* last error text of this ctx (ctx == NULL: of the last failed tsu_init on this thread) */
const char* tsu_last_error(const tsu_ctx* ctx);
/* run on the caller's hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = null stream */
int tsu_set_stream(tsu_ctx* ctx, void* hip_stream);
int tsu_synchronize(tsu_ctx* ctx);
int tsu_device_info(tsu_ctx* ctx, char* name, int name_len, int* compute_units, uint64_t* hbm_bytes);
/* hipEvent pair on the ctx stream: begin records, end records + synchronises and returns elapsed ms */
int tsu_timer_begin(tsu_ctx* ctx);
int tsu_timer_end(tsu_ctx* ctx, float* elapsed_ms);
/* n Philox4x32-10 blocks evaluated ON THE DEVICE (known-answer tests): ctrs n*4, key 2, out n*4 */
int tsu_philox4x32_10(tsu_ctx* ctx, int n, const uint32_t* ctrs, const uint32_t* key, uint32_t* out);

/* ------------------------------------------------------------------ 2-D lattice (K1, K4)
 * Replaces, for IsingGrid-shaped problems, the dense path
 *   IsingGrid.__init__           tsu/models/ising.py:320-361   (lattice instead of an N x N matrix)
 *   IsingModel.sample            tsu/models/ising.py:150-181
 *   GibbsSampler.gibbs_sweep     tsu/gibbs.py:128-162          (one call of tsu_ising2d_sweep)
 *   GibbsSampler.sample_conditional / _compute_local_field / _sigmoid   tsu/gibbs.py:61-126
 *   IsingModel.energy / magnetization   tsu/models/ising.py:99-117,183-193  (tsu_ising2d_observables)
 * Visiting order is red-black checkerboard (colour (row+col)&1 == 0 first), not raster order: the
 * same heat-bath kernel and stationary distribution, a different trajectory.
 */

/* Host helper: acceptance thresholds table[deg*5 + up] in [0, 2^32] for coupling J, uniform field h,
 * temperature T (gibbs.py:61-77,125 with ising.py:138,148 folded in).  Pure host arithmetic. */
int tsu_ising2d_thresholds(double J, double h, double T, int mode, uint64_t table[25]);

/* A whole rows x cols lattice on one GPU.  periodic needs even rows, cols >= 4 (2-colourability). */
int tsu_ising2d_create(tsu_ctx* ctx, int rows, int cols, int periodic, tsu_ising2d** out);
/* A row slab [row0, row0+rows) of a total_rows x cols lattice with `ghost` ghost rows on each side
 * that the host refreshes from the neighbouring ranks (see tsu_ising2d_row_ptr).  ghost must be even
 * and >= 2; at most ghost/2 sweeps may run between two refreshes. */
int tsu_ising2d_create_slab(tsu_ctx* ctx, int64_t total_rows, int cols, int periodic, int64_t row0, int rows,
                            int ghost, tsu_ising2d** out);
int tsu_ising2d_destroy(tsu_ising2d* lat);

/* +-1 int8 spins, row-major, `cols` bytes per row, local rows [row_first, row_first + n_rows) */
int tsu_ising2d_set_spins(tsu_ising2d* lat, const int8_t* host, int row_first, int n_rows);
int tsu_ising2d_get_spins(tsu_ising2d* lat, int8_t* host, int row_first, int n_rows);
/* i.i.d. +-1 from Philox (replaces np.random.randint(0,2,N), gibbs.py:201, for lattices too big to stage) */
int tsu_ising2d_randomize(tsu_ising2d* lat, uint64_t seed, uint32_t replica);
int tsu_ising2d_fill(tsu_ising2d* lat, int8_t value);

/* thresholds used by the following sweeps: explicit table, or J/h/T/mode through the helper above.
 * T is a per-call quantity because callers mutate config.temperature in place (gibbs.py:382). */
int tsu_ising2d_set_thresholds(tsu_ising2d* lat, const uint64_t table[25]);
int tsu_ising2d_set_model(tsu_ising2d* lat, double J, double h, double T, int mode);
int tsu_ising2d_set_kernel(tsu_ising2d* lat, int kernel, int sweeps_per_launch);

/* n_sweeps full checkerboard sweeps, sweep counters sweep0 .. sweep0+n_sweeps-1 (asynchronous); sweep0 + n_sweeps <= 2^31,
 * replica < 2^24 (so for every entry point below that takes them).
 * For a slab: ghost rows must be fresh on entry and n_sweeps <= ghost/2. */
int tsu_ising2d_sweep(tsu_ising2d* lat, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica);

/* Split form of tsu_ising2d_sweep for slabs, so the host can overlap the halo exchange with compute:
 * TSU_PART_INTERIOR updates the tile rows that do not read ghost rows (may run while ghosts are in flight and
 * does not publish anything); TSU_PART_BOUNDARY updates the remaining tile rows and publishes the new state
 * (after it, tsu_ising2d_row_ptr / get_spins see the swept lattice).  Call INTERIOR then BOUNDARY with the same
 * arguments; TSU_PART_ALL is tsu_ising2d_sweep.  TSU_E_UNSUPPORTED when the lattice is not on the tiled kernel. */
#define TSU_PART_ALL 0
#define TSU_PART_INTERIOR 1
#define TSU_PART_BOUNDARY 2
int tsu_ising2d_sweep_part(tsu_ising2d* lat, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica, int part);

/* sum_s = sum of spins, sum_bonds = sum over nearest-neighbour bonds of s_i*s_j (owned rows; the bond to
 * the row below the slab is included when that row exists).  M = sum_s/N, E = -J*sum_bonds - h*sum_s. */
int tsu_ising2d_observables(tsu_ising2d* lat, int64_t* sum_s, int64_t* sum_bonds);

/* The sampling loop of IsingModel.sample / GibbsSampler.sample_boltzmann (ising.py:150-181, gibbs.py:203-211) on the
 * lattice: n_burnin sweeps, then n_samples x (n_sweeps sweeps, record).  samples_host receives n_samples * rows * cols
 * spins (row-major, no padding).  Sweep numbers count on from sweep0; the states are gathered on the device and cross
 * PCIe once. */
int tsu_ising2d_sample(tsu_ising2d* lat, int n_burnin, int n_sweeps, int n_samples, uint64_t seed, uint32_t sweep0,
                       uint32_t replica, int8_t* samples_host);

/* Many independent lattices at once (one per temperature of a scan, ising.py:424-476; replicas of a tempering
 * ladder): lattice i does n_sweeps sweeps with its own thresholds, seeds[i], sweep0s[i], replicas[i] -- the same
 * results as n calls of tsu_ising2d_sweep.  Lattices of one shape and boundary that all run on the one-workgroup kernel
 * (TSU_KERNEL_SMALL) run as ONE launch, one workgroup each; any other batch goes to a few side streams and runs side by
 * side as far as it fits the chip together.  observables_batch: one synchronisation for all. */
int tsu_ising2d_sweep_batch(tsu_ising2d* const* lats, int n_lats, int n_sweeps, const uint64_t* seeds,
                            const uint32_t* sweep0s, const uint32_t* replicas);
int tsu_ising2d_observables_batch(tsu_ising2d* const* lats, int n_lats, int64_t* sum_s, int64_t* sum_bonds);

/* device address of local row r in [-ghost, rows+ghost) and the row pitch in bytes, for halo exchange
 * by the host (RCCL send/recv through torch.distributed on the same stream) */
int tsu_ising2d_row_ptr(tsu_ising2d* lat, int local_row, void** device_ptr, size_t* pitch_bytes);
/* Per-call timing (off by default: two event records per call cost ~2 % at 8 launches per call).  With timing on,
 * tsu_ising2d_last_sweep_ms returns the milliseconds of the most recent tsu_ising2d_sweep (HIP events; synchronises). */
int tsu_ising2d_set_timing(tsu_ising2d* lat, int enable);
int tsu_ising2d_last_sweep_ms(tsu_ising2d* lat, float* ms);
/* sweep-kernel launches issued for this lattice so far (a tile-resident launch runs many generations of sweeps) */
int tsu_ising2d_launch_count(tsu_ising2d* lat, uint64_t* n_launches);
/* Read-only view of the tile-resident kernel's strip numbering (no reference counterpart: lets a test see that it crossed a
 * restart).  *generation: generations numbered so far in the running numbering (0 before the first tile-resident launch);
 * *restarts: how often a numbering started at 1 over a cleared strip buffer: the first tile-resident launch, every launch that
 * would have reached generation 16383, and every change of the strip layout (tile shape, sweeps per generation). */
int tsu_ising2d_strip_numbering(tsu_ising2d* lat, uint32_t* generation, uint64_t* restarts);

/* ------------------------------------------------------------------ Swendsen-Wang cluster steps (K6)
 * No reference counterpart (the reference has local updates only).  One step samples exp(J sum_<ij> s_i s_j / T) at zero
 * field: every bond (right and down neighbour; wrap bonds on a periodic lattice) with J s_i s_j > 0 is active with probability
 * p = 1 - exp(-2|J|/T); the connected components of the active bonds are labelled by their smallest site index row*cols + col;
 * every cluster flips with probability 1/2, decided once at that root.  Random words: step t, site
 * (r, c): W = Philox(c >> 1, r, t, TAG_SW_BOND | replica << 8), key = seed; right bond active iff J s s' > 0 and
 * W[2 (c & 1)] < thr, down bond likewise with W[2 (c & 1) + 1]; the cluster rooted at (r, c) flips iff the top bit of word
 * c & 3 of Philox(c >> 2, r, t, TAG_SW_FLIP | replica << 8) is set.  The spins after n steps are therefore a deterministic
 * function of (spins, J, T, seed, step0, replica), whatever the launch geometry.
 * Whole lattices only (a slab: TSU_E_UNSUPPORTED); T <= 0: TSU_E_INVALID; J = 0 is legal (every site its own cluster).
 * Heat-bath sweeps and cluster steps may be interleaved; they share the spins and nothing else.  Asynchronous like the
 * sweeps: a union / find loop that hits its iteration cap is reported by the next call that synchronises. */
/* thr = floor(p 2^32), p = -expm1(-2|J|/T) in float64 (may equal 2^32).  Pure host arithmetic. */
int tsu_ising2d_cluster_threshold(double J, double T, uint64_t* thr);
/* n_steps steps with step counters step0 .. step0+n_steps-1.  A lattice of at most 16384 sites: all steps in ONE launch of
 * one workgroup (the lattice in LDS); larger ones: three launches per step (tile-local labels, merge across tile edges,
 * resolve + flip). */
int tsu_ising2d_cluster_sweep(tsu_ising2d* lat, double J, double T, int n_steps, uint64_t seed, uint32_t step0,
                              uint32_t replica);
/* the same for n_lats lattices (a temperature scan); lattices of one shape and boundary that all take the one-workgroup
 * kernel run as ONE launch, one workgroup each; otherwise one call per lattice.  Same results as n_lats calls. */
int tsu_ising2d_cluster_sweep_batch(tsu_ising2d* const* lats, int n_lats, int n_steps, const double* Js, const double* Ts,
                                    const uint64_t* seeds, const uint32_t* step0s, const uint32_t* replicas);
/* cluster-kernel launches issued for this lattice so far (separate from tsu_ising2d_launch_count) */
int tsu_ising2d_cluster_launch_count(tsu_ising2d* lat, uint64_t* n_launches);

/* ------------------------------------------------------------------ K7: quenched disorder on the lattice
 * Per-bond couplings and per-site fields for heat-bath sweeps of a whole lattice (physical mode).  Row-major (rows, cols)
 * fp32 arrays: J_right[r, c] is the bond (r, c)-(r, c+1) (wrapping to column 0 on a periodic lattice), J_down[r, c] the bond
 * (r, c)-(r+1, c) (wrapping to row 0), h[r, c] the field of site (r, c).  Decision rule:
 * f = (((J_down[r-1,c] s_up + J_down[r,c] s_down) + J_right[r,c-1] s_left) + J_right[r,c] s_right) + h[r,c] in float64 (a
 * missing neighbour of an open lattice skipped), x = 2 f / T, p = sigmoid(x) clamped at +-20, thr = floor(p 2^32 + 1/2);
 * the site becomes +1 iff u < thr, u = K1's 32-bit site uniform (same counters and tags as tsu_ising2d_sweep).  The spins
 * stay those of the handle: set_spins / get_spins / randomize / fill / observables and K1 / K6 calls keep working. */
/* Copy the disorder to the device (buffers allocated on first use, freed by tsu_ising2d_destroy).  h == NULL: zero field.
 * Non-finite values, or a nonzero J_right in the last column / J_down in the last row of an open lattice: TSU_E_INVALID.
 * A slab: TSU_E_UNSUPPORTED.  Synchronous. */
int tsu_ising2d_set_disorder(tsu_ising2d* lat, const float* J_right, const float* J_down, const float* h);
/* Forget the disorder (tsu_ising2d_disorder_sweep / _energy refuse until the next set_disorder). */
int tsu_ising2d_clear_disorder(tsu_ising2d* lat);
/* n_sweeps sweeps at temperature T with sweep counters sweep0 .. sweep0+n_sweeps-1: colour 0 ((r + c) even), then colour 1,
 * one launch per half-sweep.  Asynchronous. */
int tsu_ising2d_disorder_sweep(tsu_ising2d* lat, double T, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica);
/* E = -sum_bonds J_b s_i s_j - sum_i h_i s_i in float64, summed in a fixed order (the same bits on every call). */
int tsu_ising2d_disorder_energy(tsu_ising2d* lat, double* E);
/* q = sum_i s^a_i s^b_i of two whole lattices of one shape and context (disorder or not). */
int tsu_ising2d_overlap(tsu_ising2d* a, tsu_ising2d* b, int64_t* q);
/* K7 sweep-kernel launches issued for this lattice so far (separate from tsu_ising2d_launch_count) */
int tsu_ising2d_disorder_launch_count(tsu_ising2d* lat, uint64_t* n_launches);

/* ------------------------------------------------------------------ K7: parallel tempering (replica exchange) on one disorder
 * Replaces, for a disordered lattice, GibbsSampler.parallel_tempering tsu/gibbs.py:238-338.  n_ladders (1 or 2) ladders of n_temps
 * (2 .. 256) walkers; every walker is a whole K7 lattice (any shape tsu_ising2d_create takes), all share ONE disorder.  Walker w of
 * ladder k has Philox key seed + k n_temps + w, replica 0, the shared sweep counter, and starts at slot (temperature) w: without
 * swaps a walker is model k n_temps + w of temperature_scan(seed=seed) bit for bit.  A round (tsu_pt2d_run) = swap_interval K7
 * sweeps of every walker at the temperature of its slot, every walker's energy (the bits of tsu_ising2d_disorder_energy), then per
 * ladder one swap pass in the reference's order (gibbs.py:309-323): for i = 0 .. n_temps-2, a / b = the walkers at slots i / i+1,
 * delta = (1/T_i - 1/T_{i+1}) (E_a - E_b) in float64 (the reference writes E_b - E_a, which inverts the detailed-balance ratio),
 * accept iff delta >= 0 or u < exp(delta), u = the 53-bit uniform of
 * Philox(i >> 1, 0, t, TAG_PT_SWAP | k << 8) with key seed (t = the round counter); an accepted swap exchanges the two walkers'
 * slots, never their spins.  Round trips: a walker reaching slot 0 becomes "bottom" (the walker starting there starts so), a bottom
 * walker reaching the last slot becomes "top", a top walker reaching slot 0 counts one round trip.  DESIGN.md section 3. */
typedef struct tsu_pt2d tsu_pt2d;
int tsu_pt2d_create(tsu_ctx* ctx, int rows, int cols, int periodic, int n_temps, int n_ladders, tsu_pt2d** out);
int tsu_pt2d_destroy(tsu_pt2d* pt);
/* the same arrays, validation and messages as tsu_ising2d_set_disorder; stored once for all walkers */
int tsu_pt2d_set_disorder(tsu_pt2d* pt, const float* J_right, const float* J_down, const float* h);
/* T[slot], n_temps values, each > 0 and finite */
int tsu_pt2d_set_temperatures(tsu_pt2d* pt, const double* T);
/* initial 0: every walker from tsu_ising2d_randomize(seed + its index); +1 / -1: all up / down.  Resets slots, counters, statistics. */
int tsu_pt2d_init(tsu_pt2d* pt, uint64_t seed, int initial);
/* n_rounds rounds, all enqueued (no synchronisation).  do_swap = 0: sweeps only, no swap pass.  record: after each round's pass, per
 * slot, E (float64) and sum s (int64) of the walker there, which walker it is, and with two ladders q = sum s^a s^b of the two
 * ladders' walkers at that slot (the rows of this run replace those of the previous one). */
int tsu_pt2d_run(tsu_pt2d* pt, int n_rounds, int swap_interval, int do_swap, int record);
/* the rows of the last run: E, M, walker [round][ladder][slot]; q [round][slot] (two ladders); any pointer may be NULL */
int tsu_pt2d_history(tsu_pt2d* pt, double* E, int64_t* M, int64_t* q, int32_t* walker);
/* attempts, accepts [ladder][pair]; round_trips [ladder][walker]; walker_at_slot [ladder][slot]; any pointer may be NULL */
int tsu_pt2d_stats(tsu_pt2d* pt, int64_t* attempts, int64_t* accepts, int64_t* round_trips, int32_t* walker_at_slot,
                   uint64_t* sweep_count, uint64_t* round_count);
/* every walker's E and sum of spins now, indexed [ladder][walker] (synchronises) */
int tsu_pt2d_energies(tsu_pt2d* pt, double* E, int64_t* sum_s);
/* spins of the walker now at (ladder, slot): rows x cols int8, row-major */
int tsu_pt2d_get_spins(tsu_pt2d* pt, int ladder, int slot, int8_t* host);
int tsu_pt2d_set_spins(tsu_pt2d* pt, int ladder, int slot, const int8_t* host);
/* sweep-kernel launches so far (one per half-sweep for all walkers) */
int tsu_pt2d_launch_count(tsu_pt2d* pt, uint64_t* n_launches);

/* Replica cluster moves (Houdayer's isoenergetic cluster move) between the two ladders' walkers at one slot; needs n_ladders = 2.
 * One pass, per participating slot i, a / b = the walkers of ladder 0 / 1 now at slot i, q_x = a_x b_x: the sites with q = -1 are
 * joined to their right and down lattice neighbours with q = -1 (wrapping on a periodic lattice; whatever J is on the bond); the
 * cluster whose smallest site index r cols + c is (r, c) flips in BOTH walkers iff bit 31 of word c & 3 of
 * Philox(c >> 2, r, m, TAG_PT_ICM | slot << 8) is set, key = the seed of tsu_pt2d_init, m = the handle's cluster-pass counter (0 at
 * init, + 1 per pass, one value for all slots of a pass).  E_a + E_b and every q_x are unchanged, so no accept / reject step exists.
 * The pass helps only while the q = -1 sites do not percolate (site threshold 0.593 of the square lattice); above it one cluster
 * spans the lattice and the pass comes close to exchanging the two walkers: hence t_max and the statistics.  DESIGN.md section 3.
 *
 * every = 0 (the state after create): off, tsu_pt2d_run is what it was, launch for launch.  every >= 1: round t (the handle's round
 * counter) ends its sweeps with a pass iff t % every == 0, before the energies.  A slot takes part iff T[slot] <= t_max (t_max > 0;
 * +inf: every slot).  The setting survives tsu_pt2d_init; tsu_pt2d_set_temperatures re-evaluates which slots take part.  Switching
 * the move off drops its statistics. */
int tsu_pt2d_set_cluster_moves(tsu_pt2d* pt, int every, double t_max);
/* one pass now over the participating slots (counter m, then m + 1), enqueued, no synchronisation */
int tsu_pt2d_cluster_move(tsu_pt2d* pt);
/* per slot since init: passes taken, clusters found, sites flipped (per walker); flipped / (passes rows cols) near 1/2 says the
 * q = -1 sites percolate at that slot.  pass_count = m; n_launches = cluster-kernel launches (1 per pass for lattices of at most
 * 16384 sites, else 3; not counted by tsu_pt2d_launch_count).  Any pointer may be NULL.  Synchronises. */
int tsu_pt2d_cluster_stats(tsu_pt2d* pt, int64_t* passes, int64_t* clusters, int64_t* flipped, uint64_t* pass_count,
                           uint64_t* n_launches);

/* ------------------------------------------------------------------ K8: 3-D lattice with quenched disorder
 * No reference counterpart (the reference's IsingGrid is 2-D).  Heat-bath sweeps of a whole depth x rows x cols (D x R x C) cubic
 * lattice of +-1 int8 spins with per-bond couplings and per-site fields, physical mode.  Site (z, r, c), row-major with c fastest.
 * fp32 arrays of shape (D, R, C): J_right[z,r,c] couples (z,r,c)-(z,r,c+1), J_down[z,r,c] couples (z,r,c)-(z,r+1,c),
 * J_layer[z,r,c] couples (z,r,c)-(z+1,r,c), h[z,r,c] is the site's field.  periodic_mask has one bit per axis; a periodic axis
 * wraps to index 0 and must have an even length >= 4 (2-colourability; length 2 would make a double bond: TSU_E_UNSUPPORTED);
 * on an open axis the last slice of that axis's J must be 0 (TSU_E_INVALID otherwise).  D R < 2^31, C <= 2^30.
 * Decision rule (bit-exact):
 *   colour of a site = (z + r + c) & 1; sweep t = half-sweep hs = 2 t (colour 0), then hs = 2 t + 1 (colour 1);
 *   f = ((((((J_layer[z-1] s[z-1]) + J_layer[z] s[z+1]) + J_down[r-1] s[r-1]) + J_down[r] s[r+1]) + J_right[c-1] s[c-1])
 *       + J_right[c] s[c+1]) + h in float64, in this order, a neighbour missing on an open axis skipped (no +0.0);
 *   x = 2 f / T, p = sigmoid(x) clamped at +-20, thr = floor(p 2^32 + 1/2); the site becomes +1 iff u < thr;
 *   u = K1's 32-bit site uniform with the global row rho = z R + r in place of r: hi16 / lo16 from
 *       Philox(c >> 4, rho, hs, TAG_ISING_HI / TAG_ISING_LO | replica << 8), key = seed, halves and the flipped top bit as in K7.
 * With D = 1 and an open z axis the rule is K7's: the spins equal tsu_ising2d_disorder_sweep's bit for bit. */
#define TSU_PERIODIC_Z 1
#define TSU_PERIODIC_R 2
#define TSU_PERIODIC_C 4
typedef struct tsu_ising3d tsu_ising3d;
int tsu_ising3d_create(tsu_ctx* ctx, int depth, int rows, int cols, int periodic_mask, tsu_ising3d** out);
int tsu_ising3d_destroy(tsu_ising3d* lat);
/* +-1 int8 spins of the whole lattice, (D, R, C) row-major, no padding.  Synchronous. */
int tsu_ising3d_set_spins(tsu_ising3d* lat, const int8_t* host);
int tsu_ising3d_get_spins(tsu_ising3d* lat, int8_t* host);
/* the spins tsu_ising2d_randomize gives a (D R) x C lattice, reshaped (asynchronous) */
int tsu_ising3d_randomize(tsu_ising3d* lat, uint64_t seed, uint32_t replica);
int tsu_ising3d_fill(tsu_ising3d* lat, int8_t value);
/* Copy the disorder to the device (buffers allocated on first use, freed by tsu_ising3d_destroy).  h == NULL: zero field.
 * Non-finite values, or a nonzero last slice of an open axis's J: TSU_E_INVALID.  Synchronous. */
int tsu_ising3d_set_disorder(tsu_ising3d* lat, const float* J_right, const float* J_down, const float* J_layer, const float* h /*nullable*/);
/* n_sweeps sweeps at temperature T with sweep counters sweep0 .. sweep0+n_sweeps-1, one launch per half-sweep.  Asynchronous. */
int tsu_ising3d_sweep(tsu_ising3d* lat, double T, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica);
/* E = -sum_bonds J_b s_i s_j - sum_i h_i s_i in float64, summed in an order that depends on the shape only (the same bits on
 * every call). */
int tsu_ising3d_energy(tsu_ising3d* lat, double* E);
int tsu_ising3d_sum_spins(tsu_ising3d* lat, int64_t* sum_s);
/* q = sum_i s^a_i s^b_i of two lattices of one shape and context */
int tsu_ising3d_overlap(tsu_ising3d* a, tsu_ising3d* b, int64_t* q);
/* k8_sweep launches issued for this lattice so far */
int tsu_ising3d_launch_count(tsu_ising3d* lat, uint64_t* n_launches);

/* K8: Swendsen-Wang cluster steps on the 3-D handle (tsu_ising3d_cluster_sweep / _cluster_sweep_batch / _cluster_launch_count):
 * declared in tsu_hip_ising3d_cluster.h, which this header includes; its prototypes are _hip.CLUSTER3D_SIGNATURES in Python. */
#include "tsu_hip_ising3d_cluster.h"

/* ------------------------------------------------------------------ K8: parallel tempering of 3-D lattices on one disorder
 * tsu_pt2d for cubic lattices: n_ladders (1 or 2) ladders of n_temps (2 .. 256) walkers, every walker a whole K8 lattice (any
 * shape and periodic_mask tsu_ising3d_create takes, with its validation and messages), all sharing ONE disorder.  Walker w of
 * ladder k has Philox key seed + k n_temps + w, replica 0, the shared sweep counter, the initial draw of tsu_ising3d_randomize,
 * and starts at slot (temperature) w: without swaps a walker is model k n_temps + w of temperature_scan_3d(seed=seed) bit for
 * bit.  A round (tsu_pt3d_run) = swap_interval K8 sweeps of every walker at the temperature of its slot (one launch per
 * half-sweep for all walkers), every walker's energy (the bits of tsu_ising3d_energy), then per ladder the swap pass of
 * tsu_pt2d_run, rule, uniforms (TAG_PT_SWAP | k << 8, key = seed, counter = the round counter) and round-trip bookkeeping
 * unchanged, then the record.  No new Philox tag.  Argument meanings, array layouts and error codes are those of the
 * tsu_pt2d_* counterparts; spins are (D, R, C) int8 row-major.  An allocation that does not fit returns TSU_E_NOMEM and leaves
 * nothing behind.  DESIGN.md section 3. */
typedef struct tsu_pt3d tsu_pt3d;
int tsu_pt3d_create(tsu_ctx* ctx, int depth, int rows, int cols, int periodic_mask, int n_temps, int n_ladders, tsu_pt3d** out);
int tsu_pt3d_destroy(tsu_pt3d* pt);
/* the same arrays, validation and messages as tsu_ising3d_set_disorder; stored once for all walkers */
int tsu_pt3d_set_disorder(tsu_pt3d* pt, const float* J_right, const float* J_down, const float* J_layer, const float* h /*nullable*/);
int tsu_pt3d_set_temperatures(tsu_pt3d* pt, const double* T);
int tsu_pt3d_init(tsu_pt3d* pt, uint64_t seed, int initial);
int tsu_pt3d_run(tsu_pt3d* pt, int n_rounds, int swap_interval, int do_swap, int record);
int tsu_pt3d_history(tsu_pt3d* pt, double* E, int64_t* M, int64_t* q, int32_t* walker);
int tsu_pt3d_stats(tsu_pt3d* pt, int64_t* attempts, int64_t* accepts, int64_t* round_trips, int32_t* walker_at_slot,
                   uint64_t* sweep_count, uint64_t* round_count);
int tsu_pt3d_energies(tsu_pt3d* pt, double* E, int64_t* sum_s);
int tsu_pt3d_get_spins(tsu_pt3d* pt, int ladder, int slot, int8_t* host);
int tsu_pt3d_set_spins(tsu_pt3d* pt, int ladder, int slot, const int8_t* host);
/* k8_pt_sweep launches so far (one per half-sweep for all walkers of all ladders) */
int tsu_pt3d_launch_count(tsu_pt3d* pt, uint64_t* n_launches);

/* K7 / K8: axis profiles and k_min Fourier modes for the correlation length (tsu_ising2d_profiles / tsu_ising3d_profiles and the
 * ladders' set_correlation / history_modes / profiles): declared in tsu_hip_correlation.h, which this header includes; its
 * prototypes are _hip.CORRELATION_SIGNATURES in Python. */
#include "tsu_hip_correlation.h"

/* K7 / K8: population annealing of disordered lattices with the resampling on the device (the tsu_pa2d and tsu_pa3d handles):
 * declared in tsu_hip_population.h, which this header includes; its prototypes are _hip.POPULATION_SIGNATURES in Python. */
#include "tsu_hip_population.h"

/* K7 / K8: the link overlap of two replicas (lattice pairs, two-ladder tempering handles) and the overlaps of a population's walker
 * pairs: declared in tsu_hip_overlap.h, which this header includes; its prototypes are _hip.OVERLAP_SIGNATURES in Python. */
#include "tsu_hip_overlap.h"

/* K7 / K8: tempering ensembles, the ladders of many disorder samples in one handle and one launch per pass (the tsu_pte2d and
 * tsu_pte3d handles): declared in tsu_hip_ensemble.h, which this header includes; its prototypes are _hip.ENSEMBLE_SIGNATURES in
 * Python. */
#include "tsu_hip_ensemble.h"

/* K5: walker batches on a sparse graph, many tempering ladders or annealing restarts of one tsu_sparse graph per launch (the
 * tsu_sparse_batch handle): declared in tsu_hip_sparse_batch.h, which this header includes; its prototypes are
 * _hip.SPARSE_BATCH_SIGNATURES in Python. */
#include "tsu_hip_sparse_batch.h"

/* K7 / K8: a probe of the two numbers of the heat-bath kernels' fp32 screen, for tests of its error bound: declared in
 * tsu_hip_probe.h, which this header includes; its prototypes are _hip.PROBE_SIGNATURES in Python. */
#include "tsu_hip_probe.h"

/* K8: ghost-spin Swendsen-Wang steps, the cluster steps of the 3-D handle in a field (tsu_ising3d_cluster_sweep_field /
 * _cluster_sweep_field_batch): declared in tsu_hip_cluster_field.h, which this header includes; its prototypes are
 * _hip.CLUSTER_FIELD_SIGNATURES in Python. */
#include "tsu_hip_cluster_field.h"

/* K9: multispin-coded sweeps of the bimodal Edwards-Anderson glass, 64 disorder samples per word (tsu_msc_*): declared in
 * tsu_hip_multispin.h, which this header includes; its prototypes are _hip.MULTISPIN_SIGNATURES in Python. */
#include "tsu_hip_multispin.h"

/* K9: parallel tempering of a multispin-coded glass, per-sample swaps and the masked exchange on the device (tsu_msc_pt_*):
 * declared in tsu_hip_multispin_pt.h, which this header includes; its prototypes are _hip.MULTISPIN_PT_SIGNATURES in Python. */
#include "tsu_hip_multispin_pt.h"

/* K9: axis profiles and k_min modes of the overlap field of a multispin-coded glass, on the handle and in the tempering record
 * (tsu_msc_profiles / _set_correlation / _modes / _pt_history_modes): declared in tsu_hip_multispin_corr.h, which this header
 * includes; its prototypes are _hip.MULTISPIN_CORR_SIGNATURES in Python. */
#include "tsu_hip_multispin_corr.h"

/* K9: real-space correlations C4(r) of the overlap field along the periodic axes, plane snapshots with their two-time
 * correlations, and quench runs that record both with the measurements on the device (tsu_msc_c4 / _snapshot_slots / _snapshot /
 * _snapshot_overlap / _quench_run / _quench_history): declared in tsu_hip_multispin_quench.h, which this header includes; its
 * prototypes are _hip.MULTISPIN_QUENCH_SIGNATURES in Python. */
#include "tsu_hip_multispin_quench.h"

/* K10: q-state Potts lattices in 2-D on a handle of their own, heat-bath sweeps, Swendsen-Wang steps and exact integer observables
 * (tsu_potts2d_*): declared in tsu_hip_potts.h, which this header includes; its prototypes are _hip.POTTS_SIGNATURES in Python. */
#include "tsu_hip_potts.h"

/* K10 in 3-D: the same on the cubic lattice, one periodic flag per axis (tsu_potts3d_*): declared in tsu_hip_potts3d.h, which this
 * header includes; its prototypes are _hip.POTTS3D_SIGNATURES in Python. */
#include "tsu_hip_potts3d.h"

/* K11: multicanonical (flat-histogram) walkers of a Potts lattice, thousands of independent copies that share one weight table
 * ln W[n_eq] and add to one exact histogram (tsu_potts_muca_*): declared in tsu_hip_potts_muca.h, which this header includes; its
 * prototypes are _hip.POTTS_MUCA_SIGNATURES in Python. */
#include "tsu_hip_potts_muca.h"

/* K12: Potts lattices with per-bond couplings and per-site colour fields, 2-D and 3-D on one handle: heat-bath sweeps, Swendsen-Wang
 * steps on non-negative couplings, integer observables and a float64 energy (tsu_potts_dis_*): declared in
 * tsu_hip_potts_disorder.h, which this header includes; its prototypes are _hip.POTTS_DISORDER_SIGNATURES in Python. */
#include "tsu_hip_potts_disorder.h"

/* K13: parallel tempering of K12's lattices, one or two ladders of walkers on one disorder with the swap pass, the record and the
 * two ladders' contingency tables on the device (tsu_potts_pt_*): declared in tsu_hip_potts_pt.h, which this header includes; its
 * prototypes are _hip.POTTS_PT_SIGNATURES in Python. */
#include "tsu_hip_potts_pt.h"

/* K14: population annealing of K12's lattices, a fixed-size population of walkers on one disorder with the resampling, the record
 * and the sweeps of several walkers per workgroup on the device (tsu_potts_pop_*): declared in tsu_hip_potts_pop.h, which this
 * header includes; its prototypes are _hip.POTTS_POP_SIGNATURES in Python. */
#include "tsu_hip_potts_pop.h"

/* K6 / K8: cluster-size records of the Swendsen-Wang steps, the exact integers behind the improved estimators
 * (tsu_isingNd_cluster_measure / _cluster_record): declared in tsu_hip_cluster_measure.h, which this header includes; its prototypes
 * are _hip.CLUSTER_MEASURE_SIGNATURES in Python. */
#include "tsu_hip_cluster_measure.h"

/* ------------------------------------------------------------------ multi-GPU: RCCL below the ABI
 * One process per GPU.  A lattice that does not fit (or should not be swept by) one GPU is cut into row slabs
 * (tsu_ising2d_create_slab); these entry points refresh the ghost rows from the neighbouring ranks with RCCL send/recv over
 * xGMI and sum observables over the ranks -- no PyTorch involved (tsu/distributed.py offers the same through torch.distributed).
 * RCCL is dlopen'ed on first use.  The reference has no counterpart (it is a single Python thread). */
/* 128 opaque bytes, created on ONE rank and handed to the others by the caller (file, environment, MPI, torch.distributed ...) */
int tsu_comm_unique_id(uint8_t id[128]);
/* collective: every rank calls it with the same id; the communicator works on ctx's device and stream */
int tsu_comm_create(tsu_ctx* ctx, int nranks, int rank, const uint8_t id[128], tsu_comm** out);
int tsu_comm_destroy(tsu_comm* comm);
/* ghost rows of slab `rank` <- boundary rows of ranks rank-1 / rank+1 (wrapping for a periodic lattice), one RCCL group on the
 * ctx stream; asynchronous like the sweeps it is ordered with.  The slab must be rows * nranks == total_rows, row0 == rows * rank. */
int tsu_ising2d_halo_exchange(tsu_ising2d* lat, tsu_comm* comm);
/* values[i] <- sum over ranks (n <= 8; observables: sum of spins, sum over bonds); synchronises */
int tsu_comm_allreduce_i64(tsu_comm* comm, int64_t* values, int n);
/* Wait until everything issued on the context's stream (sweeps and halo exchanges) has finished, for at most timeout_s seconds:
 * an exchange whose peer never arrives returns TSU_E_RCCL instead of blocking for ever (the caller leaves with a non-zero exit).
 * *n_exchanges (may be NULL): halo exchanges issued by this communicator so far. */
int tsu_comm_wait(tsu_comm* comm, double timeout_s, uint64_t* n_exchanges);

/* ------------------------------------------------------------------ dense coupling matrix (K2)
 * Replaces GibbsSampler.gibbs_sweep / sample_boltzmann / compute_energy on a dense J
 *   tsu/gibbs.py:79-100 (_compute_local_field incl. the diagonal term), :102-126, :128-162, :215-236.
 * Visiting order is the reference's: range(n), or the caller's permutation (np.random.permutation).
 * State is {0,1} int8 on the device; the Python layer converts to the caller's dtype.
 */
int tsu_dense_create(tsu_ctx* ctx, int n, const void* J_host, int dtype, const double* bias_host /*nullable*/,
                     tsu_dense** out);
int tsu_dense_destroy(tsu_dense* d);
int tsu_dense_set_state(tsu_dense* d, const int8_t* bits_host);
int tsu_dense_get_state(tsu_dense* d, int8_t* bits_host);
/* order: NULL or n_sweeps*n site indices.  replay_uniforms: NULL (Philox doubles keyed by site and
 * sweep0+s) or n_sweeps*n doubles consumed in visiting order (replays np.random.rand, gibbs.py:126). */
int tsu_dense_sweep(tsu_dense* d, double T, int n_sweeps, const int64_t* order, uint64_t seed, uint32_t sweep0,
                    uint32_t replica, const double* replay_uniforms);
/* tsu_dense_sweep, _sample, _anneal and _sweep_replicas (per replica): sweep0 + all sweeps of the call <= 2^32, replica < 2^24;
 * otherwise TSU_E_INVALID ("... sweep counter overflow") before anything is launched. */
/* The whole sampling run of GibbsSampler.sample_boltzmann (tsu/gibbs.py:196-213) from the resident state:
 * n_burnin sweeps, then n_samples x (n_sweeps sweeps, record the state).  samples_host receives n_samples*n bits.
 * order / replay_uniforms cover all (n_burnin + n_samples*n_sweeps) sweeps, row per sweep; sweep numbers for the
 * Philox stream count on from sweep0.  Systems of n <= 192 (fp32 J; 128 for fp64 J) sites in natural order run as ONE launch of a single
 * wave (the reference's published benchmark sizes: n = 1 and n = 10); larger ones loop tsu_dense_sweep on the device
 * side and copy the samples back once. */
int tsu_dense_sample(tsu_dense* d, double T, int n_burnin, int n_sweeps, int n_samples, const int64_t* order,
                     uint64_t seed, uint32_t sweep0, uint32_t replica, const double* replay_uniforms,
                     int8_t* samples_host);
/* The loop of GibbsSampler.simulated_annealing (tsu/gibbs.py:366-391) from the resident state: step s does ONE sweep
 * at temperatures[s] and records the state; states_host receives n_steps*n bits (the caller evaluates the energies
 * and keeps the best, with the reference's own expression).  order / replay_uniforms: one row per step.  n <= 192 (fp32 J; 128 for fp64) in
 * natural order: one launch of a single wave for the whole schedule. */
int tsu_dense_anneal(tsu_dense* d, const double* temperatures, int n_steps, const int64_t* order, uint64_t seed,
                     uint32_t sweep0, uint32_t replica, const double* replay_uniforms, int8_t* states_host);
/* The replica loop of GibbsSampler.parallel_tempering (tsu/gibbs.py:300-306): replica r does n_sweeps sweeps of its own
 * state (states_host[r*n .. ], in and out) at temperatures[r] with its own seed / sweep counter / replica id;
 * replay_uniforms: NULL or n_replicas * n_sweeps * n doubles.  The handle's resident state is not used.  n <= 192 (fp32 J; 128 for fp64): one
 * launch, one wave per replica; up to 576 (448) sites one workgroup per replica; from 2048 sites on (a multiple of 4) up to eight
 * replicas advance together in one launch of the owner-computes kernel on ONE stream of J (groups of eight one after the other).
 * Up to eight replicas' fields stay on the device: a state that comes back byte for byte as one the previous call returned -- in
 * any position, as after a tempering swap -- resumes from that state's fields instead of a pass over J. */
int tsu_dense_sweep_replicas(tsu_dense* d, int n_replicas, const double* temperatures, int n_sweeps, int8_t* states_host,
                             const uint64_t* seeds, const uint32_t* sweep0s, const uint32_t* replicas,
                             const double* replay_uniforms);
/* -1/2 s^T J s - b^T s of the resident state (from the fields the last sweep call kept for it, or -- a state set with
 * tsu_dense_set_state that the last replica call returned -- from that replica's kept fields; otherwise one pass over J) */
int tsu_dense_energy(tsu_dense* d, double* energy);
/* the same for n_states given states (states_host: n_states x n bytes of 0/1; the resident state is not touched): the energies of
 * the states an annealing schedule recorded (simulated_annealing, gibbs.py:384-391, evaluates compute_energy after every step);
 * states the last replica call returned are evaluated from their kept fields */
int tsu_dense_energies(tsu_dense* d, const int8_t* states_host, int n_states, double* energies_host);
/* launches of the one-launch kernels this system has made so far (counts[0]: owner-computes kernel k2_own, counts[1]: pipeline
 * k2_pipe) -- lets a caller or a test see which path its sweeps took (no reference counterpart) */
int tsu_dense_launch_counts(tsu_dense* d, uint64_t counts[2]);

/* ------------------------------------------------------------------ sparse coupling graph, colour-parallel (K5)
 * Replaces GibbsSampler.gibbs_sweep / sample_boltzmann / compute_energy (tsu/gibbs.py:79-236) for models whose
 * coupling matrix is sparse -- IsingChain (tsu/models/ising.py:265-304) and IsingModel on an arbitrary graph
 * (:39-97) at sizes where the dense N x N matrix of the reference cannot exist (a 10^6-site chain would be 8 TB).
 * The graph comes as CSR (row i: columns col_idx[row_ptr[i] .. row_ptr[i+1]) ascending, bit couplings `values`, the
 * diagonal entry J_ii allowed: gibbs.py:97 includes it in the local field) plus a proper colouring: `order` lists the
 * sites colour by colour, color_offsets[c] .. color_offsets[c+1] delimit colour c in it, and no two sites of one colour
 * are coupled.  A sweep visits the colours in order and updates all sites of a colour at once -- the same outcome as
 * the reference's sequential loop run in the visiting order `order` (sites of one colour do not read each other).
 * Decision rule, field (float64) and the Philox uniform keyed by (site, sweep) are those of the dense path (K2).
 */
int tsu_sparse_create(tsu_ctx* ctx, int n, const int64_t* row_ptr /*n+1*/, const int32_t* col_idx, const double* values,
                      const double* bias_host /*nullable, n*/, int n_colors, const int32_t* color_offsets /*n_colors+1*/,
                      const int32_t* order /*n*/, tsu_sparse** out);
int tsu_sparse_destroy(tsu_sparse* g);
int tsu_sparse_set_state(tsu_sparse* g, const int8_t* bits_host); /* n bits {0,1}, site order */
int tsu_sparse_get_state(tsu_sparse* g, int8_t* bits_host);
/* sweep and sample: sweep0 + all sweeps of the call <= 2^32, replica < 2^24 (TSU_E_INVALID otherwise, nothing launched) */
int tsu_sparse_sweep(tsu_sparse* g, double T, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica);
/* n_burnin sweeps, then n_samples x (n_sweeps sweeps, record): samples_host receives n_samples*n bits (site order) */
int tsu_sparse_sample(tsu_sparse* g, double T, int n_burnin, int n_sweeps, int n_samples, uint64_t seed, uint32_t sweep0,
                      uint32_t replica, int8_t* samples_host);
/* -1/2 s^T J s - b^T s of the resident state, and sum_i (2 s_i - 1) (the magnetisation numerator in spin language) */
int tsu_sparse_energy(tsu_sparse* g, double* energy, int64_t* sum_spins);

/* Which kernel a colour class takes (no reference counterpart: lets a caller or a test see the route of its sweeps).  A PLAN record is
 * ten int32: route (0 = the generic kernel k5_color, 1 = the stencil kernels of regular classes, 2 = the whole system in one
 * workgroup, k5_small), deg, lo, hi (irregular rows at either end of the class), site_stride, pair (0 = none, 1 = prepares the
 * decisions of class `other`, 2 = consumes them), other (-1 without a pair), v4 (1 = four positions per thread), o_lo, o_n (pair = 1:
 * the partner's leading irregular rows and the number of its regular rows).  A class that is not regular leaves the other fields 0
 * and other -1; route 2 (n <= 32768) keeps what the classifier found for the class, with v4 = 0: no stencil kernel is launched.
 * tsu_sparse_classify is pure host arithmetic (no context, no GPU): the validation and the classifier of tsu_sparse_create on the
 * same arguments, under the switches TSU_K5_STENCIL, TSU_K5_PAIR, TSU_K5_V4 as they stand; plan receives n_colors records.  On
 * failure the message is tsu_last_error(NULL).  tsu_sparse_class_plan returns the record of one class of a live handle: what the
 * next sweep launches for it (TSU_K5_V4 is read at every launch). */
#define TSU_SPARSE_PLAN_LEN 10
int tsu_sparse_classify(int n, const int64_t* row_ptr, const int32_t* col_idx, const double* values, const double* bias_host /*nullable*/,
                        int n_colors, const int32_t* color_offsets, const int32_t* order, int32_t* plan /*n_colors*10*/);
int tsu_sparse_class_plan(tsu_sparse* g, int color, int32_t* rec /*10*/);

/* ------------------------------------------------------------------ Langevin (K3)
 * Replaces ThermalSamplingUnit._langevin_step (tsu/core.py:64-80) fused with the analytic gradient of a
 * separable quadratic energy E = 1/2 sum_i k_i (x_i - mu_i)^2 (replacing _numerical_gradient, :82-98),
 * for n_chains independent chains (the restarts of sample_from_energy, :140-159), float32 on the device.
 */
int tsu_langevin_create(tsu_ctx* ctx, int n_chains, int dim, tsu_langevin** out);
int tsu_langevin_destroy(tsu_langevin* l);
int tsu_langevin_set_state(tsu_langevin* l, const float* x_host);               /* n_chains*dim */
int tsu_langevin_get_state(tsu_langevin* l, float* x_host);
int tsu_langevin_set_energy(tsu_langevin* l, const float* k_host, const float* mu_host); /* dim each */
/* COUPLED quadratic energy E = 1/2 x^T A x + b^T x: A_host dim*dim row-major and SYMMETRIC (checked), b_host dim or NULL.
 * The gradient A x + b replaces _numerical_gradient (tsu/core.py:82-98) for the reference's multivariate callers
 * (tsu/api.py:94); dim <= 65536.  tsu_langevin_step then makes one launch per step (every new element needs the whole old
 * state); restart / set_state / get_state / trajectories as for the separable energy. */
int tsu_langevin_set_coupling(tsu_langevin* l, const float* A_host, const float* b_host);
/* GAUSSIAN-MIXTURE energy E(x) = -log(sum_i exp(a_i(x)) + eps), a_i(x) = log w_i - ||x - mu_i||^2 inv_var_i / 2: the reference's
 * multimodal demo (tsu/demos.py:73-87) and MultimodalSampler (tsu/api.py:143-149), whose gradient replaces _numerical_gradient
 * (tsu/core.py:82-98).  centers n_components*dim row-major, log_w and inv_var (= 1 / sigma_i^2 > 0) n_components each, log_eps = log eps
 * (-INFINITY: eps = 0); weights are NOT renormalised.  1 <= n_components <= 64, dim <= 65536; non-finite inputs refused.
 * Evaluated in the log domain: m = max_i a_i, r_i = exp(a_i - m), Z = sum_i r_i + exp(log_eps - m),
 * grad E = sum_i r_i inv_var_i (x - mu_i) / Z.  tsu_langevin_step then runs every step of a call in ONE launch (split by
 * tsu_langevin_set_kernel as for the separable energy), with the separable kernel's noise stream and update expression;
 * restart / set_state / get_state / trajectories unchanged.  A later set_energy / set_coupling switches the handle back. */
int tsu_langevin_set_mixture(tsu_langevin* l, int n_components, const float* centers, const float* log_w, const float* inv_var,
                             float log_eps);
/* x <- x_init + amp * N(0,1) per chain (core.py:142-143); chain c uses Philox chain id chain0+c */
int tsu_langevin_restart(tsu_langevin* l, const float* x_init_host /*dim*/, float amp, uint64_t seed,
                         uint32_t chain0);
/* n_steps fused steps, step counters step0.. ; traj_host (nullable): n_steps*n_chains*dim floats */
int tsu_langevin_step(tsu_langevin* l, int n_steps, float dt, float gamma, float T, uint64_t seed, uint32_t step0,
                      uint32_t chain0, float* traj_host);
int tsu_langevin_set_kernel(tsu_langevin* l, int steps_per_launch); /* 0 = auto (fuse in registers) */

#ifdef __cplusplus
}
#endif
#endif /* TSU_HIP_H */
