// What the route planner and the dispatcher (gemm.hip) need from the kernel families, without any device code: the tile constants
// the planner's rules are written in, and one host launcher per family (the instantiation ladder for a planned route).
#pragma once
#include "gemm.h"

constexpr int V5_BM = 256, V5_BN = 320, V5_BK = 32;    // gemm5.hip / conv6.hip (the other V5 constants: gemm5_epilogue.h)
constexpr int V7_BM = 256, V7_K = 320, V7_NB = 80;     // gemm7.hip
// plain GEMMs with at most this many workgroups take the producer/consumer kernel (measured at B=1: 256 -> 169.3, 512 -> 167.8,
// 768 -> 166.2, 1280 -> 164.8 steps/s)
constexpr int V4_MAX_BLOCKS = 256;

// p: the parameters as gemm_run fixed them up for the route; pl: the plan; grid: (pl.grid_x, 1, pl.grid_z).  Launch only: the caller
// reads hipGetLastError.  (hidden: internal to the library, its exported symbols stay what they were)
#pragma GCC visibility push(hidden)
void gemm3_launch(const GemmParams& p, const GemmPlan& pl, dim3 grid, hipStream_t s);   // gemm3.hip: GR_GEMM3 and GR_GEMM4
void gemm5_launch(const GemmParams& p, const GemmPlan& pl, dim3 grid, hipStream_t s);   // gemm5.hip: GR_GEMM5 and GR_UPCONV's kernel
void conv6_launch(const GemmParams& p, const GemmPlan& pl, dim3 grid, hipStream_t s);   // conv6.hip: GR_CONV6
void gemm7_launch(const GemmParams& p, const GemmPlan& pl, dim3 grid, hipStream_t s);   // gemm7.hip: GR_GEMM7
#pragma GCC visibility pop
