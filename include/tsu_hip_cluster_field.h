/* tsu_hip_cluster_field.h -- Swendsen-Wang cluster steps of the 3-D lattice handle in a field: every site has one more bond, to a
 * ghost spin fixed at +1 (csrc/ising3d_cluster.hip, the ghost instantiations of its kernels).
 *
 * Part of the C ABI of libtsu_hip.so: included by tsu_hip.h after tsu_hip_probe.h (inside its extern "C" block); include
 * tsu_hip.h, not this file.  Its ctypes prototypes are tsu._hip.CLUSTER_FIELD_SIGNATURES, one to one.
 */
#ifndef TSU_HIP_CLUSTER_FIELD_H
#define TSU_HIP_CLUSTER_FIELD_H
#ifndef TSU_HIP_H
#error "include tsu_hip.h, which includes this header"
#endif

/* ------------------------------------------------------------------ K8: ghost-spin Swendsen-Wang steps
 * n_steps cluster steps at temperature T on the stored per-bond couplings AND the stored per-site field: the step of
 * tsu_ising3d_cluster_sweep (tsu_hip_ising3d_cluster.h: the same bonds, words, tags, labels and coins) plus, for step t, key = seed,
 * global row rho = z rows + r, site index i = rho cols + c:
 *   the ghost bond of site i with stored fp32 field h_i is active iff h_i s_i > 0 and u_g < thr(|h_i|),
 *   thr(x) = floor(-expm1(-2 x / T) 2^32) in float64 from the fp32 value widened (it can be 2^32: a 64-bit compare; h_i = 0 is never
 *   active); u_g = word c & 3 of Philox(c >> 2, rho, t, TAG_SW_GHOST | replica << 8), TSU_TAG_SW_GHOST = 12;
 *   a component that contains an active ghost bond is frozen: its spins stay and it draws no coin; every other component flips by
 *   the coin of its smallest site index, as at zero field.
 * The step samples exp(-E / T) / Z for E = -sum_bonds J s s' - sum_i h_i s_i.  With an all-zero or NULL field the spins are those of
 * tsu_ising3d_cluster_sweep bit for bit.  A one-layer lattice (depth 1, open z) is the 2-D model in a field.
 * Routes and launches as at zero field (at most 16384 sites: one launch per call; larger: three per step, two without seams), counted
 * in tsu_ising3d_cluster_launch_count; the steps share the handle's cluster step counter with the zero-field ones (the caller passes
 * step0).  Errors: those of tsu_ising3d_cluster_sweep without the refusal of a field.  Asynchronous. */
int tsu_ising3d_cluster_sweep_field(tsu_ising3d* lat, double T, int n_steps, uint64_t seed, uint32_t step0, uint32_t replica);
/* The same for n_lats distinct lattices of one context, each with its own disorder, T, seed, step counter and replica id: one launch
 * when all share shape and boundary and have at most 16384 sites, otherwise one call per lattice; the same results either way. */
int tsu_ising3d_cluster_sweep_field_batch(tsu_ising3d* const* lats, int n_lats, int n_steps, const double* Ts,
                                          const uint64_t* seeds, const uint32_t* step0s, const uint32_t* replicas);

#endif /* TSU_HIP_CLUSTER_FIELD_H */
