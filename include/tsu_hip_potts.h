/* tsu_hip_potts.h -- K10: q-state Potts lattices in 2-D, heat-bath sweeps and Swendsen-Wang steps on a handle of their own
 * (csrc/potts2d.hip: potts_host.h at DIM = 2).  The categorical counterpart of the two-valued lattice handle: the reference names such cells in
 * ThermalSamplingUnit.sample_categorical (tsu/core.py) and has no lattice of them.
 *
 * Part of the C ABI of libtsu_hip.so: included by tsu_hip.h (inside its extern "C" block); include tsu_hip.h, not this file.  Its
 * ctypes prototypes are tsu._hip.POTTS_SIGNATURES, one to one.
 *
 * Model: site (r, c) holds a colour s in 0 .. q - 1 (int8, row-major), 2 <= q <= 8.  E = -J n_eq - sum_c h_c N_c, n_eq the bonds
 * whose two ends agree, N_c the sites of colour c; J one float64 of either sign, h q float64 values.  A periodic lattice needs even
 * rows and columns; a periodic axis of length 2 counts its double bond twice; an open lattice has any shape.
 */
#ifndef TSU_HIP_POTTS_H
#define TSU_HIP_POTTS_H
#ifndef TSU_HIP_H
#error "include tsu_hip.h, which includes this header"
#endif

typedef struct tsu_potts2d tsu_potts2d;

#define TSU_POTTS_MAX_Q 8
#define TSU_POTTS_RECORD_WORDS 9 /* one measurement: n_eq, N_0 .. N_7 (0 beyond q), exact int64 */

#define TSU_POTTS_HEAT_BATH 0
#define TSU_POTTS_SWENDSEN_WANG 1

#define TSU_POTTS_ROUTE_SMALL 0    /* k10_small: at most 16384 sites in one workgroup's LDS, all sweeps of a call in one launch */
#define TSU_POTTS_ROUTE_SWEEP 1    /* k10_sweep: one launch per half-sweep through HBM */
#define TSU_POTTS_ROUTE_SW_SMALL 2 /* k10_sw_small: at most 16384 sites, all steps of a call in one launch */
#define TSU_POTTS_ROUTE_SW_TILES 3 /* k10_sw_local / k10_sw_merge / k10_sw_resolve, once per step */

/* Host only (no GPU needed): TSU_OK if (q, J, h[q] or NULL for zero, T) is a model the sweeps take, else TSU_E_INVALID: q outside
 * 2 .. 8, a non-finite J, h or T, T <= 0, (4 |J| + max h - min h) / T > 600, or an exp(h_c / T) outside the float64 range (the weight
 * table stays finite and positive without a clamp).  tables (NULL, or 13 doubles): E[0 .. 4] = exp(J n / T), F[0 .. 7] = exp(h_c / T). */
int tsu_potts2d_check_model(int q, double J, const double* h, double T, double* tables);
/* Host only: the Swendsen-Wang bond threshold floor(-expm1(-J / T) 2^32) in float64 (J > 0, T > 0). */
int tsu_potts2d_cluster_threshold(double J, double T, uint64_t* thr);

/* A rows x cols lattice of q colours with its own allocation (no pad byte is ever read as a neighbour: 0 is a colour).  Refused
 * before anything is allocated: q outside 2 .. 8, rows or cols < 1, more than 2^31 - 1 sites, a periodic lattice with an odd side.
 * The model starts as J = 1, h = 0, the colours as 0. */
int tsu_potts2d_create(tsu_ctx* ctx, int rows, int cols, int q, int periodic, tsu_potts2d** out);
int tsu_potts2d_destroy(tsu_potts2d* lat);
/* J and h (q values, NULL: zero); checked as in tsu_potts2d_check_model, the temperature at every sweep */
int tsu_potts2d_set_model(tsu_potts2d* lat, double J, const double* h);
/* rows * cols colours, row-major; every value must lie in 0 .. q - 1 (TSU_E_INVALID otherwise, the lattice untouched) */
int tsu_potts2d_set_spins(tsu_potts2d* lat, const int8_t* colours);
int tsu_potts2d_get_spins(tsu_potts2d* lat, int8_t* colours);
int tsu_potts2d_fill(tsu_potts2d* lat, int colour);

/* n_sweeps checkerboard heat-bath sweeps at temperature T (asynchronous).  Colour (r + c) & 1 of sweep s is half-sweep
 * hs = 2 s + colour; the site's uniform u is the two-valued lattice's 32-bit site uniform (hi16 from TSU_TAG_ISING_HI with its top
 * bit flipped, lo16 from TSU_TAG_ISING_LO, counters (c >> 4, r, hs, tag | replica << 8), key = seed); the new colour is the smallest
 * c with (double)u Z_{q-1} < Z_c 2^32, Z the running sums of w_c = exp(J n_c / T) exp(h_c / T) in colour order (csrc/potts_dev.h,
 * DESIGN.md section 3).  The counters are 32-bit words: sweep0 is any uint32, s = sweep0 + k and hs are taken modulo 2^32 (so the
 * streams of sweeps s and s + 2^31 coincide); n_sweeps <= 2^31.  Results depend on (state, q, J, h, T, seed, sweep0, replica) only,
 * never on the route.  TSU_POTTS_SMALL=0 in the environment (tests, read per call) sends every lattice to k10_sweep. */
int tsu_potts2d_sweep(tsu_potts2d* lat, double T, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica);

/* n_steps Swendsen-Wang steps (J > 0 and h = 0; otherwise TSU_E_UNSUPPORTED and the state is untouched), step0 + n_steps <= 2^32.
 * Step t: the bond of (r, c) to its right neighbour uses word 2 (c & 1) of Philox(c >> 1, r, t, TSU_TAG_SW_BOND | replica << 8), the
 * bond to its down neighbour word 2 (c & 1) + 1; a bond is active iff its two colours agree and (uint64)u < thr
 * (tsu_potts2d_cluster_threshold).  A cluster's label is its smallest site index; the cluster rooted at (r, c) takes the colour
 * ((uint64)W q) >> 32, W = word c & 3 of Philox(c >> 2, r, t, TSU_TAG_SW_FLIP | replica << 8) (uniform to within q 2^-32).
 * TSU_SW_TILE (read per call) forces the tile edge and the tiled route, as for the two-valued lattice. */
int tsu_potts2d_cluster_sweep(tsu_potts2d* lat, double T, int n_steps, uint64_t seed, uint32_t step0, uint32_t replica);

/* TSU_POTTS_ROUTE_* a call of this algorithm would take now (the environment switches included) */
int tsu_potts2d_route(tsu_potts2d* lat, int algorithm, int* route);

/* One measurement (k10_measure; synchronises): row[0] = n_eq, row[1 + c] = N_c, exact integers by wave reductions and integer atomics */
int tsu_potts2d_measure(tsu_potts2d* lat, int64_t* row);

/* n_meas times: sweeps_between updates of `algorithm` at T, then one measurement into row k of the handle's record, all on the
 * device and without a host synchronisation.  The counters of update j of measurement k are counter0 + k sweeps_between + j, so a
 * run split in two (the second with counter0 advanced) equals one run.  The record holds the rows of the most recent run. */
int tsu_potts2d_run(tsu_potts2d* lat, double T, int n_meas, int sweeps_between, int algorithm, uint64_t seed, uint32_t counter0,
                    uint32_t replica);
/* Synchronises, sets *n_rows to the rows of the most recent run and copies min(*n_rows, max_rows) rows of TSU_POTTS_RECORD_WORDS
 * words (rows may be NULL when max_rows is 0) */
int tsu_potts2d_record(tsu_potts2d* lat, int64_t* rows, int max_rows, int* n_rows);

/* kernel launches of this handle so far (sweeps, cluster steps and measurements) */
int tsu_potts2d_launch_count(tsu_potts2d* lat, uint64_t* n);

#endif /* TSU_HIP_POTTS_H */
