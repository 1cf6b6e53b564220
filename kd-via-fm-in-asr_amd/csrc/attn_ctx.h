// Limited attention context (NeMo ConformerEncoder att_context_size / att_context_style,
// conformer_encoder.py:107-114, _create_masks :796-850) as a per-query key interval.  Query i sees the keys
// [ctx_lo(i), ctx_hi(i)] (intersected with the utterance's valid frames by the kernels):
//   chunk == 0 ("regular"):        lo = i - left (0 when left < 0),  hi = i + right (T-1 when right < 0)
//   chunk  > 0 ("chunked_limited"): c = i / chunk,  lo = (c - left) chunk (left counted in chunks; 0 when
//                                   left < 0),  hi = (c + 1) chunk - 1  (right unused)
// Both bounds are non-decreasing in i, so the keys a run of queries [i0, i1] sees lie in [lo(i0), hi(i1)] and
// the queries that see a run of keys [j0, j1] lie in [qlo(j0), qhi(j1)] -- the tile ranges the windowed kernels
// of attn_fused.hip / attn_bwd.hip walk.  The entry points clamp left / right / chunk to T (equivalent, and
// every product below stays far inside an int).
#pragma once
#include <hip/hip_runtime.h>

namespace kdfm {

struct AttnCtx {
  int left, right, chunk;
};

__host__ __device__ inline int ctx_lo(const AttnCtx c, int i) {
  if (c.left < 0) return 0;
  const int v = c.chunk > 0 ? (i / c.chunk - c.left) * c.chunk : i - c.left;
  return v > 0 ? v : 0;
}
__host__ __device__ inline int ctx_hi(const AttnCtx c, int i, int T) {
  const int v = c.chunk > 0 ? (i / c.chunk + 1) * c.chunk - 1 : (c.right < 0 ? T - 1 : i + c.right);
  return v < T - 1 ? v : T - 1;
}
// the inverse window: first / last query that sees key j
__host__ __device__ inline int ctx_qlo(const AttnCtx c, int j) {
  if (c.chunk > 0) return (j / c.chunk) * c.chunk;
  const int v = c.right < 0 ? 0 : j - c.right;
  return v > 0 ? v : 0;
}
__host__ __device__ inline int ctx_qhi(const AttnCtx c, int j, int T) {
  if (c.left < 0) return T - 1;
  const int v = c.chunk > 0 ? (j / c.chunk + c.left + 1) * c.chunk - 1 : j + c.left;
  return v < T - 1 ? v : T - 1;
}

// validated and clamped triple of an entry point (false: invalid)
inline bool ctx_make(AttnCtx& c, int32_t left, int32_t right, int32_t chunk, int64_t T) {
  if (left < -1 || right < -1 || chunk < 0) return false;
  const int t = (int)T;
  c.left = left > t ? t : left;
  c.right = right > t ? t : right;
  c.chunk = chunk > t ? t : chunk;
  return true;
}

}  // namespace kdfm
