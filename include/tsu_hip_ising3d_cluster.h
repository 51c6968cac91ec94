/* tsu_hip_ising3d_cluster.h -- the Swendsen-Wang entry points of the 3-D lattice handle (csrc/ising3d_cluster.hip).
 *
 * Part of the C ABI of libtsu_hip.so: included by tsu_hip.h after the tsu_ising3d declarations (inside its extern "C" block); include
 * tsu_hip.h, not this file.  Its ctypes prototypes are tsu._hip.CLUSTER3D_SIGNATURES, one to one.
 */
#ifndef TSU_HIP_ISING3D_CLUSTER_H
#define TSU_HIP_ISING3D_CLUSTER_H
#ifndef TSU_HIP_H
#error "include tsu_hip.h, which includes this header"
#endif

/* ------------------------------------------------------------------ K8: Swendsen-Wang cluster steps in 3-D
 * n_steps cluster steps at temperature T and zero field on the stored per-bond couplings (either sign; a uniform coupling is the
 * constant-array case).  Step t (step0 .. step0 + n_steps - 1), key = seed, global row rho = z rows + r, site index i = rho cols + c
 * (DESIGN.md section 3):
 *   a bond b = (i, j) with stored fp32 coupling J_b is active iff J_b s_i s_j > 0 and u_b < thr_b, thr_b = floor(p_b 2^32),
 *   p_b = -expm1(-2 |J_b| / T) in float64 from the fp32 value widened (J_b = 0 is never active);
 *   u_b of the right and down bonds of (z, r, c): W = Philox(c >> 1, rho, t, TAG_SW_BOND | replica << 8), right W[2 (c & 1)], down
 *   W[2 (c & 1) + 1]; of the layer bond to (z + 1, r, c) (to z = 0 across a periodic z axis): word c & 3 of
 *   Philox(c >> 2, rho, t, TAG_SW_LAYER | replica << 8), TSU_TAG_SW_LAYER = 10;
 *   labels = connected components of the active bonds, root = the smallest site index; the cluster rooted at (rho, c) flips iff
 *   bit 31 of word c & 3 of Philox(c >> 2, rho, t, TAG_SW_FLIP | replica << 8) is set.
 * The spins after n steps are a function of (spins, disorder, T, seed, step0, replica) only, whatever the route or tile shape; a
 * one-layer lattice (depth 1, open z) with constant J takes tsu_ising2d_cluster_sweep's steps on rows x cols bit for bit.
 * A lattice of at most 16384 sites runs all steps of a call in one launch; a larger one takes three launches per step.
 * Errors: a nonzero stored field: TSU_E_UNSUPPORTED (a field would need a ghost spin); depth rows cols >= 2^31: TSU_E_UNSUPPORTED;
 * T <= 0: TSU_E_INVALID ("Temperature must be positive"); no disorder set: TSU_E_INVALID.  n_steps = 0 launches nothing.
 * Heat-bath sweeps and cluster steps may be interleaved; they share the spins and nothing else.  Asynchronous. */
int tsu_ising3d_cluster_sweep(tsu_ising3d* lat, double T, int n_steps, uint64_t seed, uint32_t step0, uint32_t replica);
/* The same for n_lats distinct lattices of one context, each with its own T, seed, step counter and replica id: one launch when all
 * share shape and boundary and have at most 16384 sites, otherwise one call per lattice; the same results either way. */
int tsu_ising3d_cluster_sweep_batch(tsu_ising3d* const* lats, int n_lats, int n_steps, const double* Ts, const uint64_t* seeds,
                                    const uint32_t* step0s, const uint32_t* replicas);
/* cluster-kernel launches issued for this lattice so far (separate from tsu_ising3d_launch_count) */
int tsu_ising3d_cluster_launch_count(tsu_ising3d* lat, uint64_t* n_launches);

#endif /* TSU_HIP_ISING3D_CLUSTER_H */
