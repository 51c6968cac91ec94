// potts3d.hip -- K10 in 3-D: q-state Potts lattices on the cubic lattice, on a handle of their own (gfx950): heat-bath sweeps,
// Swendsen-Wang steps and exact integer observables (include/tsu_hip_potts3d.h; the contracts are DESIGN.md section 3).  The code is
// written once for both dimensions: the kernels in potts_kern_dev.h, the host side in potts_host.h.  This file instantiates them at
// DIM = 3 (six neighbours, one periodic flag per axis, K8's tiles and seams) behind the 3-D entry points.
#include "potts_host.h"

struct tsu_potts3d : PottsHandle<3> {};

extern "C" {

int tsu_potts3d_check_model(int q, double J, const double* h, double T, double* tables) { return potts_check_model<6>(q, J, h, T, tables); }

int tsu_potts3d_create(tsu_ctx* ctx, int depth, int rows, int cols, int q, int pz, int pr, int pc, tsu_potts3d** out) {
    return potts_create(ctx, depth, rows, cols, q, pz, pr, pc, out);
}
int tsu_potts3d_destroy(tsu_potts3d* L) { return potts_destroy(L); }
int tsu_potts3d_set_model(tsu_potts3d* L, double J, const double* h) { return potts_set_model(L, J, h); }
int tsu_potts3d_set_spins(tsu_potts3d* L, const int8_t* colours) { return potts_set_spins(L, colours); }
int tsu_potts3d_get_spins(tsu_potts3d* L, int8_t* colours) { return potts_get_spins(L, colours); }
int tsu_potts3d_fill(tsu_potts3d* L, int colour) { return potts_fill(L, colour); }
int tsu_potts3d_sweep(tsu_potts3d* L, double T, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica) {
    return potts_sweep(L, T, n_sweeps, seed, sweep0, replica);
}
int tsu_potts3d_cluster_sweep(tsu_potts3d* L, double T, int n_steps, uint64_t seed, uint32_t step0, uint32_t replica) {
    return potts_cluster_sweep(L, T, n_steps, seed, step0, replica);
}
int tsu_potts3d_route(tsu_potts3d* L, int algorithm, int* route) { return potts_route(L, algorithm, route); }
int tsu_potts3d_measure(tsu_potts3d* L, int64_t* row) { return potts_measure(L, row); }
int tsu_potts3d_run(tsu_potts3d* L, double T, int n_meas, int sweeps_between, int algorithm, uint64_t seed, uint32_t counter0,
                    uint32_t replica) {
    return potts_run(L, T, n_meas, sweeps_between, algorithm, seed, counter0, replica);
}
int tsu_potts3d_record(tsu_potts3d* L, int64_t* rows, int max_rows, int* n_rows) { return potts_record(L, rows, max_rows, n_rows); }
int tsu_potts3d_launch_count(tsu_potts3d* L, uint64_t* n) { return potts_launch_count(L, n); }

}  // extern "C"
