/* tsu_hip_multispin.h -- K9: multispin-coded heat-bath sweeps of the bimodal (J = +-1, zero field) Edwards-Anderson glass, 64 disorder
 * samples per 64-bit word (csrc/multispin.hip, csrc/multispin_dev.h).
 *
 * Part of the C ABI of libtsu_hip.so: included by tsu_hip.h after tsu_hip_cluster_field.h (inside its extern "C" block); include
 * tsu_hip.h, not this file.  Its ctypes prototypes are tsu._hip.MULTISPIN_SIGNATURES, one to one.
 *
 * Contract ("Multispin coding (K9)").  A plane is a (depth, rows, cols) array of uint64 in K8's row order (c
 * fastest); bit b of word-plane w belongs to sample 64 w + b, a set bit is spin +1.  Couplings are three arrays of W = ceil(S / 64)
 * such planes, J_right, J_down, J_layer, a set bit is J = -1; which bonds an open axis lacks follows from the periodic mask, not from
 * the data.  Pad bits (S not a multiple of 64) carry J = +1 and are swept like any other bit.  The handle holds n_temps x replicas x W
 * planes, plane (t, a, w) at index (t replicas + a) W + w.  Sample s of plane (t, a) takes, bit for bit, the decisions of
 * tsu_ising3d_sweep on that sample's couplings at T[t] with seed seeds[t replicas + a] and replica id 0: colour (z + r + c) & 1,
 * half-sweep hs = 2 sweep + colour, K1's site uniform with the global row z rows + r (hi16 from TSU_TAG_ISING_HI, lo16 from
 * TSU_TAG_ISING_LO only on a hi16 tie), spin +1 iff u < thr(f).  The 64 samples of a word share the site's uniform: each sample's
 * chain is the single lattice's, the samples of one word are correlated with each other, and two replicas of one sample therefore
 * live in different planes with different seeds.
 */
#ifndef TSU_HIP_MULTISPIN_H
#define TSU_HIP_MULTISPIN_H
#ifndef TSU_HIP_H
#error "include tsu_hip.h, which includes this header"
#endif

typedef struct tsu_msc tsu_msc;

#define TSU_MSC_ROUTE_AUTO 0
#define TSU_MSC_ROUTE_SMALL 1 /* one workgroup per plane, spins in LDS for all sweeps of a call: planes of at most 8192 sites */
#define TSU_MSC_ROUTE_HBM 2   /* one launch per half-sweep for all planes */

/* Host only (no GPU needed).  table[f + 6] = floor(p 2^32 + 1/2), p = sigmoid(2 f / T) clamped at +-20, for the local fields
 * f = -6 .. 6 of a +-1 glass: the formula of tsu_ising2d_thresholds.  Entries reach 2^32 at low T.  TSU_E_INVALID unless T > 0. */
int tsu_msc_thresholds(double T, uint64_t table[13]);

/* n_temps x replicas x ceil(n_samples / 64) planes of a depth x rows x cols lattice, all bits 0 (spins -1), couplings all +1.
 * replicas is 1 or 2.  route: TSU_MSC_ROUTE_AUTO takes SMALL where it fits; SMALL on a lattice it does not take is
 * TSU_E_UNSUPPORTED, like a periodic axis of odd length or of length below 4. */
int tsu_msc_create(tsu_ctx* ctx, int depth, int rows, int cols, int periodic_mask, int n_temps, int replicas, int n_samples, int route,
                   tsu_msc** out);
int tsu_msc_destroy(tsu_msc* h);
/* the route in use: TSU_MSC_ROUTE_SMALL or TSU_MSC_ROUTE_HBM */
int tsu_msc_route(tsu_msc* h, int* route);
/* packed couplings, each W x depth x rows x cols uint64 (J_layer may be NULL for depth 1) */
int tsu_msc_set_couplings(tsu_msc* h, const uint64_t* J_right, const uint64_t* J_down, const uint64_t* J_layer);
/* packed spins, (n_temps, replicas, W, depth, rows, cols) uint64 */
int tsu_msc_set_planes(tsu_msc* h, const uint64_t* planes);
int tsu_msc_get_planes(tsu_msc* h, uint64_t* planes);
/* seeds[t replicas + a]: the Philox key of plane (t, a), for randomize and sweep */
int tsu_msc_set_seeds(tsu_msc* h, const uint64_t* seeds);
/* every sample of plane (t, a) starts from tsu_ising3d_randomize(seeds[t replicas + a], replica 0) */
int tsu_msc_randomize(tsu_msc* h);
/* every spin +1 or -1 */
int tsu_msc_fill(tsu_msc* h, int8_t value);
/* T[n_temps], each > 0: uploads one 13-entry table per temperature slot (the sweep kernels contain no exp) */
int tsu_msc_set_temperatures(tsu_msc* h, const double* T);
/* n_sweeps sweeps of every plane, the first with sweep counter sweep0.  SMALL: one launch; HBM: 2 n_sweeps launches.  Asynchronous. */
int tsu_msc_sweep(tsu_msc* h, int n_sweeps, uint32_t sweep0);
/* Exact per-sample integers of every plane in one launch, W * 64 columns each (the caller drops the pad columns):
 *   unsat[(t replicas + a) 64 W + s]: unsatisfied bonds (E = 2 unsat - N_b);  sum[..]: sum of spins;
 *   with two replicas q[t 64 W + s] = sum_i a_i b_i and q_link[t 64 W + s] = sum over bonds of a_i a_j b_i b_j (NULL allowed;
 *   required NULL or ignored with one replica).  Synchronous. */
int tsu_msc_measure(tsu_msc* h, int64_t* unsat, int64_t* sum, int64_t* q, int64_t* q_link);
/* sweep-kernel launches so far */
int tsu_msc_launch_count(tsu_msc* h, uint64_t* out);

#endif /* TSU_HIP_MULTISPIN_H */
