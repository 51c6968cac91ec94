/* tsu_hip_multispin_corr.h -- K9: axis profiles and k_min Fourier modes of a multispin-coded glass (csrc/multispin_corr.hip).
 *
 * Part of the C ABI of libtsu_hip.so: included by tsu_hip.h after tsu_hip_multispin_pt.h (inside its extern "C" block); include
 * tsu_hip.h, not this file.  Its ctypes prototypes are tsu._hip.MULTISPIN_CORR_SIGNATURES, one to one.
 *
 * Contract ("Correlation length of multispin-coded glasses (K9)").  The site field of slot t and sample s is
 * f_i = a_i b_i, the two replicas at the slot, or f_i = s_i with one replica.  The profile of axis d at coordinate x is the exact
 * integer sum of f over the sites with that coordinate, P_d[x] = n_x - 2 count(bits set in a ^ b, or in ~a, on those sites),
 * n_x = N / L_d: integers only, the same on every run, every profile of a sample summing to its q N (or sum s).  Pad bits are
 * computed like any other bit (the outputs have 64 W columns).  The k_min mode of a periodic axis is
 * F_d = sum_x P_d[x] (cos_d[x] + i sin_d[x]) in float64 from the caller's tables, summed in the order of tsu_hip_correlation.h:
 * partial t of 256 adds its terms x = t, t + 256, ... in ascending order from 0.0, every product rounded before its add; the 64
 * partials of each of the four groups fold by halves; (g0 + g1) + (g2 + g3).  An open axis has a profile and no mode.
 */
#ifndef TSU_HIP_MULTISPIN_CORR_H
#define TSU_HIP_MULTISPIN_CORR_H
#ifndef TSU_HIP_H
#error "include tsu_hip.h, which includes this header"
#endif

/* The profiles of the planes as they are: p_z [n_temps][64 W][depth], p_r [n_temps][64 W][rows], p_c [n_temps][64 W][cols].  Works
 * whether the modes are switched on or not.  Synchronous. */
int tsu_msc_profiles(tsu_msc* h, int64_t* p_z, int64_t* p_r, int64_t* p_c);
/* enable != 0: the tables cos(2 pi x / L), sin(2 pi x / L) of every periodic axis, x = 0 .. L - 1; the pair of an axis is NULL
 * exactly when the axis is open (TSU_E_INVALID otherwise, and when no axis is periodic).  From then on a recording round of
 * tsu_msc_pt_run also records the modes.  enable == 0 (the state after create; the tables are ignored): every other entry point
 * enqueues exactly what it does without this header. */
int tsu_msc_set_correlation(tsu_msc* h, int enable, const double* cos_z, const double* sin_z, const double* cos_r, const double* sin_r,
                            const double* cos_c, const double* sin_c);
/* The modes of the planes as they are, [n_temps][64 W][periodic axes in axis order][re, im]: one profile launch and one mode
 * launch.  TSU_E_INVALID unless the modes are switched on.  Synchronous. */
int tsu_msc_modes(tsu_msc* h, double* modes);
/* The modes of the n_rows rounds the last tsu_msc_pt_run recorded (n_rows must be that number), each row taken with the round's
 * measurement, after its sweeps and before its swap pass: [n_rows][n_temps][64 W][periodic axes][re, im].  TSU_E_INVALID if that
 * run recorded none (modes off, or record = 0).  Synchronous. */
int tsu_msc_pt_history_modes(tsu_msc* h, int n_rows, double* modes);

#endif /* TSU_HIP_MULTISPIN_CORR_H */
