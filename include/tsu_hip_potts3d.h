/* tsu_hip_potts3d.h -- K10 in 3-D: q-state Potts lattices on the cubic lattice, heat-bath sweeps and Swendsen-Wang steps on a handle
 * of their own (csrc/potts3d.hip: potts_host.h at DIM = 3).  The 3-D counterpart of tsu_hip_potts.h, symbol for symbol, as tsu_ising3d is of
 * the two-valued 2-D lattice.
 *
 * Part of the C ABI of libtsu_hip.so: included by tsu_hip.h (inside its extern "C" block, after tsu_hip_potts.h, whose
 * TSU_POTTS_MAX_Q, TSU_POTTS_RECORD_WORDS, TSU_POTTS_HEAT_BATH and TSU_POTTS_SWENDSEN_WANG it shares); include tsu_hip.h, not this
 * file.  Its ctypes prototypes are tsu._hip.POTTS3D_SIGNATURES, one to one.
 *
 * Model: site (z, r, c) of a depth x rows x cols lattice holds a colour s in 0 .. q - 1 (int8, row-major, no pad: site index
 * i = (z rows + r) cols + c), 2 <= q <= 8.  E = -J n_eq - sum_c h_c N_c, n_eq the bonds of the three axes whose two ends agree.  One
 * periodic flag per axis (pz, pr, pc); a periodic axis has even length, and one of length 2 counts its double bond twice (in the
 * heat-bath counts, in the cluster bonds and in n_eq); an open axis has any length >= 1.  One layer is depth = 1, pz = 0: it takes
 * tsu_potts2d_sweep's and tsu_potts2d_cluster_sweep's colours on rows x cols bit for bit, on every route.
 */
#ifndef TSU_HIP_POTTS3D_H
#define TSU_HIP_POTTS3D_H
#ifndef TSU_HIP_H
#error "include tsu_hip.h, which includes this header"
#endif

typedef struct tsu_potts3d tsu_potts3d;

#define TSU_POTTS3D_ROUTE_SMALL 0    /* route k10_3d_small (kernel k10_small<3>): at most 16384 sites in one workgroup's LDS, all sweeps of a call in one launch */
#define TSU_POTTS3D_ROUTE_SWEEP 1    /* route k10_3d_sweep (k10_sweep<3>): one launch per half-sweep through HBM */
#define TSU_POTTS3D_ROUTE_SW_SMALL 2 /* route k10_3d_sw_small (k10_sw_small<3>): at most 16384 sites, all steps of a call in one launch */
#define TSU_POTTS3D_ROUTE_SW_TILES 3 /* route k10_3d_sw_tiles (k10_sw_local<3> / k10_sw_merge<3> / k10_sw_resolve<3>), once per step */

/* Host only (no GPU needed): TSU_OK if (q, J, h[q] or NULL for zero, T) is a model the sweeps take, else TSU_E_INVALID: q outside
 * 2 .. 8, a non-finite J, h or T, T <= 0, (6 |J| + max h - min h) / T > 600 (the six-neighbour bound, whatever the depth), or an
 * exp(h_c / T) outside the float64 range.  tables (NULL, or 15 doubles): E[0 .. 6] = exp(J n / T), F[0 .. 7] = exp(h_c / T). */
int tsu_potts3d_check_model(int q, double J, const double* h, double T, double* tables);

/* A depth x rows x cols lattice of q colours with its own allocation.  Refused before anything is allocated: q outside 2 .. 8, an
 * extent < 1, 2^31 sites or more, a periodic axis of odd length.  The model starts as J = 1, h = 0, the colours as 0. */
int tsu_potts3d_create(tsu_ctx* ctx, int depth, int rows, int cols, int q, int pz, int pr, int pc, tsu_potts3d** out);
int tsu_potts3d_destroy(tsu_potts3d* lat);
/* J and h (q values, NULL: zero); checked as in tsu_potts3d_check_model, the temperature at every sweep */
int tsu_potts3d_set_model(tsu_potts3d* lat, double J, const double* h);
/* depth * rows * cols colours, row-major; every value must lie in 0 .. q - 1 (TSU_E_INVALID otherwise, the lattice untouched) */
int tsu_potts3d_set_spins(tsu_potts3d* lat, const int8_t* colours);
int tsu_potts3d_get_spins(tsu_potts3d* lat, int8_t* colours);
int tsu_potts3d_fill(tsu_potts3d* lat, int colour);

/* n_sweeps checkerboard heat-bath sweeps at temperature T (asynchronous).  Colour (z + r + c) & 1 of sweep s is half-sweep
 * hs = 2 s + colour; the site's uniform is tsu_potts2d_sweep's with the global row rho = z rows + r in place of r (counters
 * (c >> 4, rho, hs, tag | replica << 8), TSU_TAG_ISING_HI and TSU_TAG_ISING_LO, key = seed); the rule is the same with up to six
 * neighbours: w_c = E[n_c] F[c], n_c = 0 .. 6 (csrc/potts_dev.h).  The counters are 32-bit words and wrap as in
 * 2-D; n_sweeps <= 2^31.  Results depend on (state, q, J, h, T, seed, sweep0, replica) only, never on the route.  TSU_POTTS_SMALL=0
 * in the environment (tests, read per call) sends every lattice to route k10_3d_sweep. */
int tsu_potts3d_sweep(tsu_potts3d* lat, double T, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica);

/* n_steps Swendsen-Wang steps (J > 0 and h = 0; otherwise TSU_E_UNSUPPORTED and the state is untouched), step0 + n_steps <= 2^32.
 * Step t: the right and down bonds of (z, r, c) use words 2 (c & 1) and 2 (c & 1) + 1 of Philox(c >> 1, rho, t, TSU_TAG_SW_BOND |
 * replica << 8); the layer bond to z + 1 (to z = 0 across a periodic z) word c & 3 of Philox(c >> 2, rho, t, TSU_TAG_SW_LAYER |
 * replica << 8); a bond is active iff its two colours agree and (uint64)u < thr (tsu_potts2d_cluster_threshold).  A cluster's label
 * is its smallest site index; the cluster rooted at (rho, c) takes the colour ((uint64)W q) >> 32, W = word c & 3 of
 * Philox(c >> 2, rho, t, TSU_TAG_SW_FLIP | replica << 8).  TSU_SW3D_TILE=<tz>x<tr>x<tc> (read per call) forces the tile shape and
 * the tiled route, as for the two-valued 3-D lattice; the default tiles are that lattice's. */
int tsu_potts3d_cluster_sweep(tsu_potts3d* lat, double T, int n_steps, uint64_t seed, uint32_t step0, uint32_t replica);

/* TSU_POTTS3D_ROUTE_* a call of this algorithm (TSU_POTTS_HEAT_BATH, TSU_POTTS_SWENDSEN_WANG) would take now */
int tsu_potts3d_route(tsu_potts3d* lat, int algorithm, int* route);

/* One measurement (k10_measure<3>; synchronises): row[0] = n_eq, row[1 + c] = N_c (TSU_POTTS_RECORD_WORDS words), exact integers */
int tsu_potts3d_measure(tsu_potts3d* lat, int64_t* row);

/* n_meas times: sweeps_between updates of `algorithm` at T, then one measurement into row k of the handle's record, all on the
 * device and without a host synchronisation.  The counters of update j of measurement k are counter0 + k sweeps_between + j, so a
 * run split in two (the second with counter0 advanced) equals one run.  The record holds the rows of the most recent run. */
int tsu_potts3d_run(tsu_potts3d* lat, double T, int n_meas, int sweeps_between, int algorithm, uint64_t seed, uint32_t counter0,
                    uint32_t replica);
/* Synchronises, sets *n_rows to the rows of the most recent run and copies min(*n_rows, max_rows) rows of TSU_POTTS_RECORD_WORDS
 * words (rows may be NULL when max_rows is 0) */
int tsu_potts3d_record(tsu_potts3d* lat, int64_t* rows, int max_rows, int* n_rows);

/* kernel launches of this handle so far (sweeps, cluster steps and measurements) */
int tsu_potts3d_launch_count(tsu_potts3d* lat, uint64_t* n);

#endif /* TSU_HIP_POTTS3D_H */
