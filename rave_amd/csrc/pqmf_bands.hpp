// PQMF direct-form transforms for the band counts other than 16 (pqmf_bands.hip); pqmf.hip routes n_band != 16 here.
#pragma once
#include "common.hpp"

// 1 iff the band count has a kernel instance here (2, 4, 8, 32)
bool rh_pqmf_bands_has(int n_band);
// frames per workgroup tile of that instance, 0 without one
int rh_pqmf_bands_tile_frames(int n_band);
// Same arguments and meaning as the public entry points of include/rave_hip.h; pointers, rows and n_band are already checked.
int rh_pqmf_bands_analysis_fwd(const float* x, const float* w, int rows, int t_len, int n_band, int kernel, int pad_left,
                               int n_frames, float* y, hipStream_t stream);
int rh_pqmf_bands_analysis_bwd(const float* dy, const float* w, int rows, int t_len, int n_band, int kernel, int pad_left,
                               int n_frames, float* dx, hipStream_t stream);
int rh_pqmf_bands_synthesis_fwd(const float* y, const float* w, int rows, int n_frames, int n_band, int kernel, int pad_left,
                                int n_out, float* x, hipStream_t stream);
int rh_pqmf_bands_synthesis_bwd(const float* dx, const float* w, int rows, int n_frames, int n_band, int kernel, int pad_left,
                                int n_out, float* dy, hipStream_t stream);
