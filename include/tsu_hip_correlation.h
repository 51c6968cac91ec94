/* tsu_hip_correlation.h -- axis profiles and k_min Fourier modes: what the second-moment correlation length needs
 * (csrc/corr_dev.h, entry points in csrc/ising2d_disorder.hip and csrc/ising3d.hip).
 *
 * Part of the C ABI of libtsu_hip.so: included by tsu_hip.h after the tsu_pt3d declarations (inside its extern "C" block); include
 * tsu_hip.h, not this file.  Its ctypes prototypes are tsu._hip.CORRELATION_SIGNATURES, one to one.
 */
#ifndef TSU_HIP_CORRELATION_H
#define TSU_HIP_CORRELATION_H
#ifndef TSU_HIP_H
#error "include tsu_hip.h, which includes this header"
#endif

/* ------------------------------------------------------------------ K7 / K8: axis profiles and k_min modes
 * Site field f = s (one lattice) or s^a s^b (two lattices of one shape, or the two ladders' walkers at one slot).  The profile of
 * an axis is the exact int64 sum of f over all sites that share a coordinate on it: 2-D P_row[r] = sum_c f, P_col[c] = sum_r f;
 * 3-D P_z[z] = sum_{r,c} f, P_r[r] = sum_{z,c} f, P_c[c] = sum_{z,r} f.  Every profile sums to sum s / q.  Integer accumulation
 * only: the same values on every run.  The k_min mode of a periodic axis of length L is F = sum_x P[x] (cos(2 pi x / L) +
 * i sin(2 pi x / L)) in float64 with the tables made on the HOST and handed in (no device cos / sin): thread t of 256 adds its
 * terms x = t, t + 256, ... in ascending order from 0.0, each product rounded before its add (no fused multiply-add), then the 64
 * lanes of each wave fold by halves (32, 16, .., 1) and the four waves add as (w0 + w1) + (w2 + w3).  An open axis has a profile
 * and no mode.  DESIGN.md section 3, "Correlation length". */
/* Profiles of lattice a (b == NULL) or of the product a b.  Whole lattices of one shape and context only (a slab:
 * TSU_E_UNSUPPORTED).  p_row: rows values, p_col: cols values.  Synchronises. */
int tsu_ising2d_profiles(tsu_ising2d* a, tsu_ising2d* b /*nullable*/, int64_t* p_row, int64_t* p_col);
/* p_z: depth, p_r: rows, p_c: cols values */
int tsu_ising3d_profiles(tsu_ising3d* a, tsu_ising3d* b /*nullable*/, int64_t* p_z, int64_t* p_r, int64_t* p_c);
/* enable != 0: every recording round of tsu_pt2d_run also records, per slot, the modes of the periodic axes of the walker there
 * (one ladder: its spins; two: the product of the two ladders' walkers), after the overlap, without waiting for the device.  The
 * tables have rows / cols doubles; an axis's pair is NULL exactly when the axis is open (TSU_E_INVALID otherwise, and when no axis
 * is periodic).  Switching it on drops the rows of the previous run.  enable == 0 (the state after create): a run enqueues what it
 * did before this entry point existed; the tables are ignored.  Synchronises. */
int tsu_pt2d_set_correlation(tsu_pt2d* pt, int enable, const double* cos_row, const double* sin_row, const double* cos_col,
                             const double* sin_col);
int tsu_pt3d_set_correlation(tsu_pt3d* pt, int enable, const double* cos_z, const double* sin_z, const double* cos_r,
                             const double* sin_r, const double* cos_c, const double* sin_c);
/* the modes of the last run's rows, [round][slot][periodic axis, in axis order][re, im]; TSU_E_INVALID if that run recorded none
 * (correlation off, or record = 0) */
int tsu_pt2d_history_modes(tsu_pt2d* pt, double* modes);
int tsu_pt3d_history_modes(tsu_pt3d* pt, double* modes);
/* the profiles of the walker(s) now at `slot`, whether correlation is on or not.  Synchronises. */
int tsu_pt2d_profiles(tsu_pt2d* pt, int slot, int64_t* p_row, int64_t* p_col);
int tsu_pt3d_profiles(tsu_pt3d* pt, int slot, int64_t* p_z, int64_t* p_r, int64_t* p_c);

#endif /* TSU_HIP_CORRELATION_H */
