/* tsu_hip_overlap.h -- the link overlap of two replicas of one disorder, and the spin / link overlaps and k_min modes of the walker
 * pairs of an annealed population (csrc/link_dev.h, csrc/pt_host.h, csrc/pop_host.h, entry points in csrc/ising2d_disorder.hip and
 * csrc/ising3d.hip).
 *
 * Part of the C ABI of libtsu_hip.so: included by tsu_hip.h after tsu_hip_population.h (inside its extern "C" block); include
 * tsu_hip.h, not this file.  Its ctypes prototypes are tsu._hip.OVERLAP_SIGNATURES, one to one.
 */
#ifndef TSU_HIP_OVERLAP_H
#define TSU_HIP_OVERLAP_H
#ifndef TSU_HIP_H
#error "include tsu_hip.h, which includes this header"
#endif

/* ------------------------------------------------------------------ K7 / K8: link overlap
 * p_i = s^a_i s^b_i.  L = sum over bonds (i, j) of p_i p_j, an exact integer; the bonds are those of the lattice's energy: every
 * site's right, down and (3-D) layer bond, the last bond of an open axis dropped, the wrap bond of a periodic axis kept (a periodic
 * axis of length 1 or 2 counts its wrap bond as the energy does).  N_b is their number; q_l = L / N_b.  Integer arithmetic only: the
 * same value on every run.  DESIGN.md section 3, "Overlaps of walker pairs". */
/* Two whole lattices of one shape, periodic flags and context (b == a is allowed: L = N_b); unequal shapes or flags:
 * TSU_E_INVALID; a slab: TSU_E_UNSUPPORTED.  Synchronises. */
int tsu_ising2d_link_overlap(tsu_ising2d* a, tsu_ising2d* b, int64_t* L, int64_t* n_bonds);
int tsu_ising3d_link_overlap(tsu_ising3d* a, tsu_ising3d* b, int64_t* L, int64_t* n_bonds);
/* enable != 0 (two ladders only, TSU_E_INVALID otherwise): every recording round of run also records, per slot, L of the two
 * ladders' walkers the swap pass left there, right after q, without waiting for the device.  Switching it on drops the rows of the
 * previous run.  enable == 0 (the state after create): a run enqueues what it did before this entry point existed. */
int tsu_pt2d_set_link_overlap(tsu_pt2d* pt, int enable);
int tsu_pt3d_set_link_overlap(tsu_pt3d* pt, int enable);
/* L of the last run's rows, [round][slot]; TSU_E_INVALID if that run recorded none.  Synchronises. */
int tsu_pt2d_history_link(tsu_pt2d* pt, int64_t* L);
int tsu_pt3d_history_link(tsu_pt3d* pt, int64_t* L);

/* ------------------------------------------------------------------ K7 / K8: overlaps of a population's walker pairs
 * Pairs are (walker i, walker i + P), i < P = population / 2 (rounded down: with an odd population the last walker has no partner).
 * enable != 0: a recording run also records, for the population it starts from (row 0) and after each step's sweeps (row j), per
 * pair q N = sum_i s^a_i s^b_i and L, and, if tables are given, the k_min modes of the pair's overlap field on the periodic axes
 * (tsu_hip_correlation.h: the same profile and mode passes, summation order included).  All tables NULL: q and L only.  Tables
 * given: an axis's (cos, sin) pair of the axis's length is NULL exactly when the axis is open (TSU_E_INVALID otherwise, and when
 * no axis is periodic).  Whether the two walkers of a pair descend from different walkers of the start is for the caller to decide
 * from `parent` (tsu_pa2d_history).  Switching it on, or changing whether modes are recorded, drops the rows of the previous run;
 * enable == 0 (the state after create): a run enqueues what it did before this entry point existed.  A buffer that does not fit:
 * TSU_E_NOMEM, nothing left behind.  Synchronises; a run with it on still waits for nothing. */
int tsu_pa2d_set_overlap(tsu_pa2d* pa, int enable, const double* cos_row, const double* sin_row, const double* cos_col,
                         const double* sin_col);
int tsu_pa3d_set_overlap(tsu_pa3d* pa, int enable, const double* cos_z, const double* sin_z, const double* cos_r, const double* sin_r,
                         const double* cos_c, const double* sin_c);
/* The overlap rows of the last run (n = its n_steps; any pointer may be NULL): q, L [n + 1][P]; modes [n + 1][P][periodic axis, in
 * axis order][re, im].  TSU_E_INVALID if that run recorded none (overlaps off, or record = 0), or modes are asked for and were not
 * recorded.  Synchronises. */
int tsu_pa2d_history_overlap(tsu_pa2d* pa, int64_t* q, int64_t* L, double* modes);
int tsu_pa3d_history_overlap(tsu_pa3d* pa, int64_t* q, int64_t* L, double* modes);

#endif /* TSU_HIP_OVERLAP_H */
