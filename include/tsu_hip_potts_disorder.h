/* tsu_hip_potts_disorder.h -- K12: q-state Potts lattices with per-bond couplings and per-site colour fields, in 2-D and 3-D, on a
 * handle of their own beside K10's (csrc/potts_disorder.hip, potts_disorder_kern_dev.h, potts_disorder_dev.h): heat-bath sweeps,
 * Swendsen-Wang steps on non-negative couplings, exact integer observables and a float64 energy.
 *
 * Part of the C ABI of libtsu_hip.so: included by tsu_hip.h (inside its extern "C" block, after tsu_hip_potts_muca.h; it shares
 * TSU_POTTS_MAX_Q, TSU_POTTS_RECORD_WORDS, TSU_POTTS_HEAT_BATH and TSU_POTTS_SWENDSEN_WANG with tsu_hip_potts.h); include tsu_hip.h,
 * not this file.  Its ctypes prototypes are tsu._hip.POTTS_DISORDER_SIGNATURES, one to one.
 *
 * Model: site (z, r, c) of a depth x rows x cols lattice holds a colour 0 .. q - 1 (int8, row-major, no pad: site index
 * i = (z rows + r) cols + c), 2 <= q <= 8.  E = -sum_bonds J_b [s_i = s_j] - sum_i h[i][s_i].  One periodic flag per axis; a periodic
 * axis has even length, and one of length 2 holds two stored bonds between its pair, which both count.  One handle serves both
 * dimensions: a lattice with depth 1 and an open z axis is 2-D and runs kernels that carry no z term.
 *
 * Disorder: fp32 arrays of the lattice's shape; the entry of J_right, J_down, J_layer at a site is the bond that leaves it in +c, +r,
 * +z (to index 0 across a periodic axis); on an open axis the last column, row or layer of that array must be 0.  The field is
 * colour-major: h[c sites + i], q planes of the lattice's shape.
 *
 * Heat-bath rule (tests/helpers/potts_disorder_twin.py is its NumPy twin): the visiting order, the octet and the
 * 32-bit site uniform u are tsu_potts3d_sweep's exactly (colour (z + r + c) & 1, hs = 2 sweep + colour mod 2^32, counters
 * (c >> 4, rho, hs, tag | replica << 8), TSU_TAG_ISING_HI and TSU_TAG_ISING_LO, key = seed).  For a site with the existing neighbours
 * k in the order z-1, z+1, r-1, r+1, c-1, c+1: a_c = (double)h[c][i] (0.0 without a field) plus (double)J_k for every neighbour, in
 * that order, that shows colour c (one rounded add each); a* = max_c a_c; w_c = exp((a_c - a*) / T) in float64; Z_c = Z_{c-1} + w_c in
 * colour order; thr_c = (uint64)floor(Z_c / Z_{q-1} 2^32 + 0.5) for c < q - 1, thr_{q-1} = 2^32; the new colour is the smallest c with
 * (uint64)u < thr_c.  Results depend on (state, q, disorder, T, seed, sweep0, replica) only, never on the route.  On constant arrays
 * the rule samples K10's distribution but is not K10's rule bit for bit.
 */
#ifndef TSU_HIP_POTTS_DISORDER_H
#define TSU_HIP_POTTS_DISORDER_H
#ifndef TSU_HIP_H
#error "include tsu_hip.h, which includes this header"
#endif

typedef struct tsu_potts_dis tsu_potts_dis;

#define TSU_POTTS_DIS_RECORD_WORDS 10   /* a record row: TSU_POTTS_RECORD_WORDS integers (n_eq, N_0 .. N_7), then the bits of E */
#define TSU_POTTS_DIS_ROUTE_SMALL 0     /* k12_small: at most 16384 sites in one workgroup's LDS, all sweeps of a call in one launch */
#define TSU_POTTS_DIS_ROUTE_SWEEP 1     /* k12_sweep: one launch per half-sweep through HBM */
#define TSU_POTTS_DIS_ROUTE_SW_SMALL 2  /* k12_sw_small: at most 16384 sites, all steps of a call in one launch */
#define TSU_POTTS_DIS_ROUTE_SW_TILES 3  /* k12_sw_local / k12_sw_merge / k12_sw_resolve, once per step */

/* Host only (no GPU needed): steps 2 - 5 of the rule for one site with the sums a[0 .. q - 1] at temperature T: thr[0 .. q - 1].
 * TSU_E_INVALID for q outside 2 .. 8, a non-finite a or T, or T <= 0. */
int tsu_potts_dis_site_thresholds(int q, const double* a, double T, uint64_t* thr);

/* A depth x rows x cols lattice of q colours; periodic: three flags (pz, pr, pc).  Refused before anything is allocated: q outside
 * 2 .. 8, an extent < 1, 2^31 sites or more, a periodic axis of odd length.  The colours start as 0; no disorder is set. */
int tsu_potts_dis_create(tsu_ctx* ctx, int depth, int rows, int cols, int q, const int* periodic, tsu_potts_dis** out);
int tsu_potts_dis_destroy(tsu_potts_dis* lat);

/* The couplings and the field (synchronous).  J_layer is NULL for a 2-D lattice (depth 1, open z; an array of zeros is accepted
 * too, as the last layer of an open axis) and required otherwise; h is q
 * colour-major planes or NULL for zero field (the sweeps then read no field plane).  Refused before anything is allocated or
 * copied: a non-finite value, a non-zero last column / row / layer of an open axis's array.  Swendsen-Wang steps are allowed
 * afterwards iff every existing bond has J >= 0 and h is NULL or all zero. */
int tsu_potts_dis_set_disorder(tsu_potts_dis* lat, const float* J_right, const float* J_down, const float* J_layer, const float* h);

/* depth * rows * cols colours, row-major; every value must lie in 0 .. q - 1 (TSU_E_INVALID otherwise, the lattice untouched) */
int tsu_potts_dis_set_spins(tsu_potts_dis* lat, const int8_t* colours);
int tsu_potts_dis_get_spins(tsu_potts_dis* lat, int8_t* colours);
int tsu_potts_dis_fill(tsu_potts_dis* lat, int colour);

/* n_sweeps checkerboard heat-bath sweeps at temperature T (asynchronous) by the rule above; T <= 0 or non-finite: TSU_E_INVALID.
 * The counters are 32-bit words and wrap; n_sweeps <= 2^31.  TSU_POTTS_SMALL=0 in the environment (tests, read per call) sends
 * every lattice to k12_sweep. */
int tsu_potts_dis_sweep(tsu_potts_dis* lat, double T, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica);

/* n_steps Swendsen-Wang steps on the stored couplings, step0 + n_steps <= 2^32.  TSU_E_UNSUPPORTED, the state untouched, when a bond
 * is negative or the field is not zero.  The words, tags, labels and the root's colour are tsu_potts3d_cluster_sweep's; a bond is
 * active iff its two colours agree and (uint64)u < floor(-expm1(-(double)J_b / T) 2^32), evaluated per satisfied bond on the device
 * (J_b = 0, a diluted bond, is never active).  TSU_SW_TILE (2-D) and TSU_SW3D_TILE (3-D) act as they do for K10. */
int tsu_potts_dis_cluster_sweep(tsu_potts_dis* lat, double T, int n_steps, uint64_t seed, uint32_t step0, uint32_t replica);

/* TSU_POTTS_DIS_ROUTE_* a call of this algorithm (TSU_POTTS_HEAT_BATH, TSU_POTTS_SWENDSEN_WANG) would take now */
int tsu_potts_dis_route(tsu_potts_dis* lat, int algorithm, int* route);

/* One measurement (k12_measure; synchronises): row[0] = n_eq, row[1 + c] = N_c (TSU_POTTS_RECORD_WORDS words, exact integers, as
 * tsu_potts3d_measure counts them) and *E (may be NULL) in float64, summed in a fixed order: the same bits on every call and route */
int tsu_potts_dis_measure(tsu_potts_dis* lat, int64_t* row, double* E);

/* n_meas times: sweeps_between updates of `algorithm` at T, then one measurement into row k of the handle's record, all on the
 * device and without a host synchronisation.  The counters of update j of measurement k are counter0 + k sweeps_between + j, so a
 * run split in two (the second with counter0 advanced) equals one run.  The record holds the rows of the most recent run. */
int tsu_potts_dis_run(tsu_potts_dis* lat, double T, int n_meas, int sweeps_between, int algorithm, uint64_t seed, uint32_t counter0,
                      uint32_t replica);
/* Synchronises, sets *n_rows to the rows of the most recent run and copies min(*n_rows, max_rows) rows of
 * TSU_POTTS_DIS_RECORD_WORDS words, the last one the bits of the float64 E (rows may be NULL when max_rows is 0) */
int tsu_potts_dis_record(tsu_potts_dis* lat, int64_t* rows, int max_rows, int* n_rows);

/* kernel launches of this handle so far (sweeps, cluster steps and measurements) */
int tsu_potts_dis_launch_count(tsu_potts_dis* lat, uint64_t* n);

#endif /* TSU_HIP_POTTS_DISORDER_H */
