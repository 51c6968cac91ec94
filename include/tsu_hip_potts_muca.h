/* tsu_hip_potts_muca.h -- K11: multicanonical (flat-histogram) walkers of a q-state Potts lattice (csrc/potts_muca.hip,
 * potts_muca_dev.h).  A handle holds `walkers` independent copies of one depth x rows x cols lattice of q colours, one shared table
 * ln W[n] over n = n_eq (the satisfied bonds, 0 .. B) and exact integer records H[n], S1[n], S2[n] that every walker adds to after
 * every sweep.
 *
 * Part of the C ABI of libtsu_hip.so: included by tsu_hip.h (inside its extern "C" block, after tsu_hip_potts3d.h); include
 * tsu_hip.h, not this file.  Its ctypes prototypes are tsu._hip.POTTS_MUCA_SIGNATURES, one to one.
 *
 * Model: site (z, r, c) holds a colour 0 .. q - 1, site index i = (z rows + r) cols + c, 2 <= q <= 8.  The walkers sample the weight
 * W(n_eq) in place of exp(-E / T); the physical energy E = -J n_eq (zero field) enters only when a record is reweighted, on the
 * host.  One periodic flag per axis; any side >= 1 is allowed, odd periodic sides included (no checkerboard, so no parity
 * constraint).  A periodic axis of length 2 contributes its double bond twice (as tsu_potts3d_measure counts it), one of length 1
 * contributes none; B is the bond count with that multiplicity.  z_max, the largest |delta n| of one update, is 4 for a one-layer
 * lattice whose depth axis is open and 6 otherwise.
 *
 * Update rule (the stream contract; tests/helpers/potts_muca_twin.py is its NumPy twin, bit for bit): sweep
 * t = sweep0 + k (mod 2^32) of walker w visits the sites in index order.  Sites i and i ^ 1 share the Philox4x32-10 block with
 * counters (i >> 1, w, t, TSU_TAG_POTTS_MUCA | replica << 8) and key = seed; word 2 (i & 1) is the proposal word P, word
 * 2 (i & 1) + 1 the acceptance uniform u.  The proposal is c' = (c + 1 + (((uint64)P (q - 1)) >> 32)) mod q, never c itself;
 * delta = n_{c'} - n_c over the existing neighbours (a double neighbour counted twice); the move is accepted iff
 * (uint64)u < thr[n][delta] with n the walker's current n_eq (tsu_potts_muca_thresholds: made on the host in float64, no exp on the
 * device).  After every sweep each walker adds H[n] += 1, S1[n] += N_max, S2[n] += N_max^2 (N_max = max_c N_c; uint64, integer
 * atomics only, so the record is exact and independent of the order) and moves its tunnel state.  Results depend on (state, q,
 * geometry, ln W, seed, sweep0, replica) only: never on the route, on how walkers are packed into workgroups or on how a run is
 * split into calls.
 */
#ifndef TSU_HIP_POTTS_MUCA_H
#define TSU_HIP_POTTS_MUCA_H
#ifndef TSU_HIP_H
#error "include tsu_hip.h, which includes this header"
#endif

typedef struct tsu_potts_muca tsu_potts_muca;

#define TSU_POTTS_MUCA_MAX_SITES 65536      /* sites of one lattice */
#define TSU_POTTS_MUCA_MAX_WALKERS 1048576  /* 2^20; also walkers * sites <= 2^31 - 1 */

/* All three routes run k11_muca, every sweep of a call in one launch, one lane per walker; they differ in where the data lives. */
#define TSU_POTTS_MUCA_ROUTE_LDS 0      /* the workgroup's lattices, the histogram and the threshold table all in LDS */
#define TSU_POTTS_MUCA_ROUTE_GLOBAL 1   /* lattices in device memory (state[site][walker]), histogram and table in LDS */
#define TSU_POTTS_MUCA_ROUTE_ATOMICS 2  /* lattices in device memory, histogram by global atomics, table gathered through L2 */

/* Host only (no GPU needed): *bonds = B and *z_max of a depth x rows x cols lattice with these periodic flags (pz, pr, pc).
 * TSU_E_INVALID for a side < 1 or more than TSU_POTTS_MUCA_MAX_SITES sites. */
int tsu_potts_muca_geometry(int depth, int rows, int cols, const int* periodic, int64_t* bonds, int* z_max);

/* Host only: the acceptance table of ln W[0 .. B], out[n (2 z_max + 1) + delta + z_max] for n = 0 .. B, delta = -z_max .. z_max:
 * 2^32 when lnw[n + delta] >= lnw[n], else floor(exp(lnw[n + delta] - lnw[n]) 2^32); 0 where n + delta lies outside 0 .. B (such
 * entries are never read).  This is the table the device decides with.  TSU_E_INVALID for B < 0, a z_max other than 4 or 6, or a
 * non-finite lnw. */
int tsu_potts_muca_thresholds(int64_t bonds, int z_max, const double* lnw, uint64_t* out);

/* Refused before anything is allocated: q outside 2 .. 8, a side < 1, more than TSU_POTTS_MUCA_MAX_SITES sites, walkers < 1 or
 * > TSU_POTTS_MUCA_MAX_WALKERS, walkers * sites > 2^31 - 1.  periodic: three flags (pz, pr, pc).  The handle starts with every
 * colour 0, ln W = 0, an empty record and the tunnel bounds (0, B). */
int tsu_potts_muca_create(tsu_ctx* ctx, int depth, int rows, int cols, int q, const int* periodic, int walkers, tsu_potts_muca** out);
int tsu_potts_muca_destroy(tsu_potts_muca* m);

/* ln W[0 .. B]; TSU_E_INVALID (weights untouched) for len != B + 1 or a non-finite entry */
int tsu_potts_muca_set_weights(tsu_potts_muca* m, const double* lnw, int64_t len);
/* walker-major (walkers, depth, rows, cols) int8 colours; every value must lie in 0 .. q - 1 (TSU_E_INVALID otherwise, the state
 * untouched).  set_spins and fill recompute n_eq and N_c of every walker on the device (k11_measure). */
int tsu_potts_muca_set_spins(tsu_potts_muca* m, const int8_t* colours);
int tsu_potts_muca_get_spins(tsu_potts_muca* m, int8_t* colours);
int tsu_potts_muca_fill(tsu_potts_muca* m, int colour);

/* Tunnel bounds, 0 <= n_lo < n_hi <= B.  After every sweep: n <= n_lo makes the walker's side low, n >= n_hi makes it high, and a
 * change from one side to the other counts one event.  Setting the bounds clears every walker's side and count. */
int tsu_potts_muca_set_tunnel_bounds(tsu_potts_muca* m, int64_t n_lo, int64_t n_hi);

/* n_sweeps sweeps of every walker with the current weights, in one launch (asynchronous); 0 <= n_sweeps <= 2^31 - 1, the sweep
 * counter sweep0 + k wraps as a 32-bit word.  The environment (read per call) may force a route and a workgroup size:
 * TSU_POTTS_MUCA_ROUTE=<r> takes route max(r, the route chosen by size); TSU_POTTS_MUCA_BLOCK=<threads> (a multiple of 64, 64 ..
 * 1024) sets the walkers per workgroup where it fits.  Neither changes a result. */
int tsu_potts_muca_run(tsu_potts_muca* m, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica);

/* n_eq of every walker (walkers int32); synchronises */
int tsu_potts_muca_energies(tsu_potts_muca* m, int32_t* n_eq);
/* tunnel events of every walker (walkers uint32); synchronises */
int tsu_potts_muca_tunnels(tsu_potts_muca* m, uint32_t* events);
/* H, S1, S2: B + 1 words each (any may be NULL); synchronises */
int tsu_potts_muca_record(tsu_potts_muca* m, uint64_t* H, uint64_t* S1, uint64_t* S2);
int tsu_potts_muca_clear_record(tsu_potts_muca* m);

/* Recomputes n_eq and N_c of every walker from the spins (k11_measure; synchronises); *equal = 1 iff all of them equalled the
 * incrementally kept ones, which are replaced either way. */
int tsu_potts_muca_measure(tsu_potts_muca* m, int* equal);

/* TSU_POTTS_MUCA_ROUTE_* a run would take now */
int tsu_potts_muca_route(tsu_potts_muca* m, int* route);
/* k11_muca launches of this handle so far (one per run with n_sweeps > 0; measurements are not counted) */
int tsu_potts_muca_launch_count(tsu_potts_muca* m, uint64_t* n);

#endif /* TSU_HIP_POTTS_MUCA_H */
