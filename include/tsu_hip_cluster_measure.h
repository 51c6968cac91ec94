/* tsu_hip_cluster_measure.h -- cluster-size records of the Swendsen-Wang steps (K6 on the 2-D handle, K8 on the 3-D handle, zero
 * field and ghost spin): the improved estimators' raw material, exact integers written on the device (csrc/sw_dev.h, sw_host.h).
 *
 * Part of the C ABI of libtsu_hip.so: included by tsu_hip.h after tsu_hip_multispin_quench.h (inside its extern "C" block); include
 * tsu_hip.h, not this file.  Its ctypes prototypes are tsu._hip.CLUSTER_MEASURE_SIGNATURES, one to one.
 */
#ifndef TSU_HIP_CLUSTER_MEASURE_H
#define TSU_HIP_CLUSTER_MEASURE_H
#ifndef TSU_HIP_H
#error "include tsu_hip.h, which includes this header"
#endif

/* One row of TSU_CLUSTER_RECORD_WORDS int64 words per cluster step, from the step's own decomposition into components of active
 * bonds (a free cluster is a component that does not reach the ghost spin; M_C = sum of s_i over the sites of C, signed):
 *   0  n_clusters  free clusters
 *   1  largest     sites of the largest free cluster
 *   2  sum_size2   sum over free clusters of |C|^2
 *   3  sum_m2      sum over free clusters of M_C^2
 *   4, 5  sum_m4   sum over free clusters of M_C^4, an unsigned 128-bit integer: low word, high word
 *   6  n_frozen    sites whose component reaches the ghost (0 on the zero-field entry points)
 *   7  m_frozen    sum of s_i over those sites
 * Integer accumulation only, so a row is the same bits on every run.  M_C^2 and m_frozen do not change under the step's own flips.
 * A step whose union / find cap expired leaves its row zero (the next synchronising call reports the error). */
#define TSU_CLUSTER_RECORD_WORDS 8

/* The switch on the handle (on != 0: on).  While it is on, every cluster entry point (tsu_ising2d_cluster_sweep / _sweep_batch,
 * tsu_ising3d_cluster_sweep / _sweep_batch / _sweep_field / _sweep_field_batch) records one row per step of that lattice; the spins
 * of every step are bit for bit those with the switch off (no random number is added).  Switching on allocates nothing until the next
 * cluster call; switching off frees nothing (a running kernel may still write the buffers, which go with the handle).  A batch takes
 * its one-launch route only if all of its lattices agree on the switch, otherwise they run one by one, with the same results.
 * Launches with the switch on: at most 16384 sites: one per call, as without; larger (or a forced tile): three more per step (the
 * counts per tile root, their fold onto the global roots, the row), two more where the lattice has no seam; all are counted in
 * tsu_isingNd_cluster_launch_count. */
int tsu_ising2d_cluster_measure(tsu_ising2d* lat, int on);
int tsu_ising3d_cluster_measure(tsu_ising3d* lat, int on);

/* The rows of the lattice's most recent measured cluster call: synchronises, sets *n_rows to the number of steps of that call (0:
 * none yet) and copies min(*n_rows, max_rows) rows of TSU_CLUSTER_RECORD_WORDS words to rows (rows may be NULL when max_rows is 0).
 * A kernel's expired cap is reported here like by any synchronising call. */
int tsu_ising2d_cluster_record(tsu_ising2d* lat, int64_t* rows, int max_rows, int* n_rows);
int tsu_ising3d_cluster_record(tsu_ising3d* lat, int64_t* rows, int max_rows, int* n_rows);

#endif /* TSU_HIP_CLUSTER_MEASURE_H */
