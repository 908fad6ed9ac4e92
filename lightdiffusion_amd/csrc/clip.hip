// CLIP text model input stage (CLIPEmbeddings, LD.py:4394-4410, with the textual-inversion table of SDClipModel.set_up_textual_embeddings,
// LD.py:4642-4690, read where it lies instead of rebuilt):
//   out[b][l] = round_fp16( float(row(ids[b][l])) + float(pos[l]) )
// row(id) = table[id] for id < V-1; extra[id - (V-1)] (fp32, the prompt's custom vectors) for V-1 <= id < V-1+E; table[V-1] (EOS, which the
// remap keeps the largest id) for id == V-1+E.  The reference copies the whole [V, h] table into a new nn.Embedding of V + E rows per prompt;
// here the resident table is never copied.  A load-class operation: B * L rows of h values, once per prompt.
#include "kernels.h"

namespace {

// one wave per output row; lane `l` owns the 8-value (16-byte) columns l, l + 64, ...
__global__ __launch_bounds__(LD_WAVE) void clip_embed_kernel(const int* __restrict__ ids, const half_t* __restrict__ table, const float* __restrict__ extra,
                                                             const half_t* __restrict__ pos, half_t* __restrict__ out, int rows, int L, int V, int E, int h) {
    const int r = blockIdx.x;
    if (r >= rows) return;
    const int id = ids[r];
    // which memory the row comes from; an id outside [0, V + E) reads NO table memory and gives a row of zeros (the host range-checks the
    // ids before upload: this guard only keeps a bad id from reading out of bounds)
    const half_t* trow = nullptr;
    const float* erow = nullptr;
    if (id >= 0 && id < V - 1) trow = table + (long long)id * h;
    else if (id >= V - 1 && id < V - 1 + E) erow = extra + (long long)(id - (V - 1)) * h;
    else if (id == V - 1 + E) trow = table + (long long)(V - 1) * h;
    const half_t* prow = pos + (long long)(r % L) * h;
    half_t* orow = out + (long long)r * h;
    for (int c = threadIdx.x * 8; c < h; c += LD_WAVE * 8) {
        float f[8];
        if (trow != nullptr) {
            unpack8(ld16(trow + c), f);
        } else if (erow != nullptr) {
            const float4 a = *reinterpret_cast<const float4*>(erow + c), b = *reinterpret_cast<const float4*>(erow + c + 4);
            f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
            f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
        } else {
            st16(orow + c, zero16());
            continue;
        }
        float p[8];
        unpack8(ld16(prow + c), p);
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] += p[i];
        st16(orow + c, pack8(f));
    }
}

}  // namespace

int clip_embed_launch(const int* ids, const half_t* table, const float* extra, const half_t* pos, half_t* out, int B, int L, int V, int E, int h,
                      hipStream_t stream) {
    if (ids == nullptr || table == nullptr || pos == nullptr || out == nullptr || (E > 0 && extra == nullptr)) return LD_ERR_ARG;
    if (B < 1 || L < 1 || V < 2 || E < 0 || h < 1) return LD_ERR_ARG;
    if (h % 8 != 0) return LD_ERR_SHAPE;
    if ((((uintptr_t)table | (uintptr_t)extra | (uintptr_t)pos | (uintptr_t)out) & 15) != 0) return LD_ERR_SHAPE;   // 16-byte loads and stores
    const long long rows = (long long)B * L;
    if (rows > 0x7fffffffLL || (long long)V + E > 0x7fffffffLL) return LD_ERR_SHAPE;
    hipLaunchKernelGGL(clip_embed_kernel, dim3((unsigned)rows), dim3(LD_WAVE), 0, stream, ids, table, extra, pos, out, (int)rows, L, V, E, h);
    return hipGetLastError() == hipSuccess ? LD_OK : LD_ERR_HIP;
}
