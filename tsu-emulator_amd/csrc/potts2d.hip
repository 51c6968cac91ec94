// potts2d.hip -- K10: q-state Potts lattices in 2-D on a handle of their own (gfx950): heat-bath sweeps, Swendsen-Wang steps and
// exact integer observables (include/tsu_hip_potts.h; the contracts are DESIGN.md section 3).  The code is written once for both
// dimensions: the kernels in potts_kern_dev.h, the host side in potts_host.h.  This file instantiates them at DIM = 2 (a lattice of
// depth 1 whose z terms are compiled out, not skipped at run time) behind the 2-D entry points.
#include "potts_host.h"

struct tsu_potts2d : PottsHandle<2> {};

extern "C" {

int tsu_potts2d_check_model(int q, double J, const double* h, double T, double* tables) { return potts_check_model<4>(q, J, h, T, tables); }

int tsu_potts2d_cluster_threshold(double J, double T, uint64_t* thr) {
    if (!thr || !(T > 0.0) || !isfinite(T) || !isfinite(J) || !(J > 0.0)) return TSU_E_INVALID;
    *thr = potts_threshold(J, T);
    return TSU_OK;
}

int tsu_potts2d_create(tsu_ctx* ctx, int rows, int cols, int q, int periodic, tsu_potts2d** out) {
    return potts_create(ctx, 1, rows, cols, q, 0, periodic, periodic, out);
}
int tsu_potts2d_destroy(tsu_potts2d* L) { return potts_destroy(L); }
int tsu_potts2d_set_model(tsu_potts2d* L, double J, const double* h) { return potts_set_model(L, J, h); }
int tsu_potts2d_set_spins(tsu_potts2d* L, const int8_t* colours) { return potts_set_spins(L, colours); }
int tsu_potts2d_get_spins(tsu_potts2d* L, int8_t* colours) { return potts_get_spins(L, colours); }
int tsu_potts2d_fill(tsu_potts2d* L, int colour) { return potts_fill(L, colour); }
int tsu_potts2d_sweep(tsu_potts2d* L, double T, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica) {
    return potts_sweep(L, T, n_sweeps, seed, sweep0, replica);
}
int tsu_potts2d_cluster_sweep(tsu_potts2d* L, double T, int n_steps, uint64_t seed, uint32_t step0, uint32_t replica) {
    return potts_cluster_sweep(L, T, n_steps, seed, step0, replica);
}
int tsu_potts2d_route(tsu_potts2d* L, int algorithm, int* route) { return potts_route(L, algorithm, route); }
int tsu_potts2d_measure(tsu_potts2d* L, int64_t* row) { return potts_measure(L, row); }
int tsu_potts2d_run(tsu_potts2d* L, double T, int n_meas, int sweeps_between, int algorithm, uint64_t seed, uint32_t counter0,
                    uint32_t replica) {
    return potts_run(L, T, n_meas, sweeps_between, algorithm, seed, counter0, replica);
}
int tsu_potts2d_record(tsu_potts2d* L, int64_t* rows, int max_rows, int* n_rows) { return potts_record(L, rows, max_rows, n_rows); }
int tsu_potts2d_launch_count(tsu_potts2d* L, uint64_t* n) { return potts_launch_count(L, n); }

}  // extern "C"
