// LoRA merge into resident weights (ModelPatcher.patch_model / calculate_weight, LD.py:3335-3354, 3407-3424, on the device):
//   dst = round_fp16( float(base) + sum_j scale_j * up_j * down_j )
// A load-class operation, bound by reading and writing W: fp32 FMAs on the vector ALUs, the up / down tiles staged in LDS as fp32.
// The accumulator STARTS at float(base) and every product of every term is one FMA onto it, so the result sees (sum of ranks) fp32
// roundings of the running sum, one of scale * up per product, and ONE rounding to fp16 (nearest) for all terms together.
// The logical (row, column) -> resident element map lives in lora_resident_index; the merge and the read-back kernel both use it.
#include "kernels.h"

namespace {

// element (r, c) of the checkpoint matrix [rows][cols] (a conv: c = i * 9 + ky * 3 + kx, the flatten(start_dim=1) of OIHW) -> its index in
// the slot's resident layout: LORA_MAT as is; LORA_CONV3 [O][ky][kx][I] (repack_conv3x3_kernel); LORA_GEGLU output tile t of bn rows =
// [bn/2 value rows t*bn/2.. | bn/2 gate rows rows/2 + t*bn/2..] (repack_rows_kernel)
__device__ __forceinline__ long long lora_resident_index(const LoraLayout& L, int r, int c) {
    if (L.kind == LORA_CONV3) {
        const int I = L.cols / 9, i = c / 9, tap = c - i * 9;
        return ((long long)r * 9 + tap) * I + i;
    }
    if (L.kind == LORA_GEGLU) {
        const int hb = L.bn / 2, half = L.rows / 2;
        const int q = r < half ? r : r - half;
        const int rd = (q / hb) * L.bn + (q % hb) + (r < half ? 0 : hb);
        return (long long)rd * L.cols + c;
    }
    return (long long)r * L.cols + c;
}

constexpr int BM = 64, BN = 64, KC = 16;   // output tile per workgroup, rank chunk per LDS stage

template <typename T>
__device__ __forceinline__ void stage_term(const LoraTerm& t, int k0, int row0, int col0, int rows, int cols, float (*us)[BM + 1], float (*ds)[BN]) {
    const T* up = static_cast<const T*>(t.up);
    const T* down = static_cast<const T*>(t.down);
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < BM * KC / 256; ++i) {          // up tile: consecutive lanes read consecutive k of one row
        const int e = tid + i * 256, r = e / KC, k = e - r * KC;
        const bool ok = row0 + r < rows && k0 + k < t.rank;
        us[k][r] = ok ? t.scale * (float)up[(long long)(row0 + r) * t.rank + k0 + k] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < BN * KC / 256; ++i) {          // down tile: consecutive lanes read consecutive columns
        const int e = tid + i * 256, k = e / BN, c = e - k * BN;
        const bool ok = col0 + c < cols && k0 + k < t.rank;
        ds[k][c] = ok ? (float)down[(long long)(k0 + k) * cols + col0 + c] : 0.f;
    }
}

// one 64 x 64 tile of the logical matrix per workgroup; thread (ty, tx) owns rows ty*4 .. +3 and columns tx, tx+16, tx+32, tx+48.
// Every element is read (base) and written (dst) by the same thread: dst may alias base.
__global__ __launch_bounds__(256) void lora_merge_kernel(const LoraArgs a) {
    __shared__ float us[KC][BM + 1];
    __shared__ float ds[KC][BN];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int row0 = blockIdx.y * BM, col0 = blockIdx.x * BN;
    const int rows = a.lay.rows, cols = a.lay.cols;
    float acc[4][4];
    long long at[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = row0 + ty * 4 + i, c = col0 + tx + 16 * j;
            const bool ok = r < rows && c < cols;
            at[i][j] = ok ? lora_resident_index(a.lay, r, c) : -1;
            acc[i][j] = ok ? (float)a.base[at[i][j]] : 0.f;
        }
    for (int j = 0; j < a.n_terms; ++j) {
        const LoraTerm& t = a.t[j];
        for (int k0 = 0; k0 < t.rank; k0 += KC) {
            __syncthreads();
            if (t.f32) stage_term<float>(t, k0, row0, col0, rows, cols, us, ds);
            else stage_term<half_t>(t, k0, row0, col0, rows, cols, us, ds);
            __syncthreads();
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                float u[4], d[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) u[i] = us[k][ty * 4 + i];
#pragma unroll
                for (int q = 0; q < 4; ++q) d[q] = ds[k][tx + 16 * q];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[i][q] = fmaf(u[i], d[q], acc[i][q]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (at[i][j] >= 0) a.dst[at[i][j]] = (half_t)acc[i][j];   // fp32 -> fp16, round to nearest even
}

__global__ void lora_read_kernel(const half_t* __restrict__ resident, const LoraLayout L, half_t* __restrict__ dst) {
    const long long total = (long long)L.rows * L.cols;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(q / L.cols), c = (int)(q - (long long)r * L.cols);
        dst[q] = resident[lora_resident_index(L, r, c)];
    }
}

int layout_status(const LoraLayout& L) {
    if (L.rows < 1 || L.cols < 1) return LD_ERR_ARG;
    if (L.kind == LORA_CONV3 && L.cols % 9) return LD_ERR_ARG;
    if (L.kind == LORA_GEGLU && (L.bn < 2 || (L.bn & 1) || L.rows % L.bn)) return LD_ERR_ARG;
    if (L.kind != LORA_MAT && L.kind != LORA_CONV3 && L.kind != LORA_GEGLU) return LD_ERR_ARG;
    return LD_OK;
}

}  // namespace

int lora_merge_launch(const LoraArgs& a, hipStream_t stream) {
    if (a.base == nullptr || a.dst == nullptr || layout_status(a.lay) != LD_OK) return LD_ERR_ARG;
    if (a.n_terms < 1 || a.n_terms > LORA_MAX_TERMS) return LD_ERR_ARG;
    for (int j = 0; j < a.n_terms; ++j)
        if (a.t[j].up == nullptr || a.t[j].down == nullptr || a.t[j].rank < 1 || a.t[j].rank > LORA_MAX_RANK) return LD_ERR_ARG;
    const dim3 grid((a.lay.cols + BN - 1) / BN, (a.lay.rows + BM - 1) / BM);
    if (grid.y > 65535u) return LD_ERR_SHAPE;
    hipLaunchKernelGGL(lora_merge_kernel, grid, dim3(256), 0, stream, a);
    return hipGetLastError() == hipSuccess ? LD_OK : LD_ERR_HIP;
}

int lora_read_launch(const half_t* resident, const LoraLayout& lay, half_t* dst, hipStream_t stream) {
    if (resident == nullptr || dst == nullptr || layout_status(lay) != LD_OK) return LD_ERR_ARG;
    const long long total = (long long)lay.rows * lay.cols;
    long long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(lora_read_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, resident, lay, dst);
    return hipGetLastError() == hipSuccess ? LD_OK : LD_ERR_HIP;
}
