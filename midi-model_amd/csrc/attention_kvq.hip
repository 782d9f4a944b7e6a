// The event-level K/V cache in 8 bits (DecodeSession(kv_dtype="fp8")): OCP e4m3fn codes with one fp32 scale per
// (sequence, head, event) for K and one for V.  Per layer the cache is
//   k8, v8  uint8 [B, H, Lmax, 64]   the codes
//   sc      fp32  [B, H, Lmax, 2]    (K scale, V scale) of that row: one 8-byte load serves a key
// -- 136 bytes per (head, event) where the bf16 cache holds 256.  Head dim 64, bf16 activations.
//
// Q(x) of a 64-element row x (bf16 values read as fp32), the ONE definition (tests/ref_kvq.py restates it in torch, bit for bit):
//   amax = max_e |x_e|;  s = amax / 448 (IEEE fp32 division), s = 1 when amax == 0;
//   code_e = e4m3fn(clamp(x_e / s, -448, 448)), round to nearest even, subnormals kept;  D(code, s)_e = float(code_e) * s.
// The clamp keeps the conversion away from its overflow behaviour: the NaN codes 0x7F / 0xFF are never produced.
//
//   mh_kv_store_seqs_rows_fp8       the packed prefill store of mh_kv_store_seqs_rows, writing Q() of every K row and V row
//   mh_attn_decode_append_rows_fp8  mh_attn_decode_append_rows over this cache: the new row is quantized, stored, and attended to
//                                   in its dequantized form, so that this event and every later one see the same key
//   mh_kv_fork_rows_fp8             mh_kv_fork_rows over this cache: codes and scales copied bit for bit
// These are kernels of their own (attention_small.hip's instantiations are what they were).
#include "common.h"

namespace {

constexpr int QHD = 64;            // head dim
constexpr float FP8_MAX = 448.f;   // the largest e4m3fn value (code 0x7E)

typedef __attribute__((ext_vector_type(2))) float kvq_f32x2;
typedef __attribute__((ext_vector_type(2))) unsigned kvq_u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned kvq_u32x4;

// s of Q(): amax / 448, 1 for an all-zero row
__device__ inline float kvq_scale(float amax) { return amax == 0.f ? 1.f : amax / FP8_MAX; }
// the clamped quotient the conversion rounds
__device__ inline float kvq_quot(float x, float s) { return fminf(fmaxf(x / s, -FP8_MAX), FP8_MAX); }
// four fp32 -> four e4m3fn codes in one dword (element 0 in the low byte): two v_cvt_pk_fp8_f32
__device__ inline unsigned kvq_pack4(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return (unsigned)w;
}
// ... and back: two v_cvt_pk_f32_fp8
__device__ inline void kvq_unpack4(unsigned w, float (&f)[4]) {
  const kvq_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  f[0] = lo[0];
  f[1] = lo[1];
  f[2] = hi[0];
  f[3] = hi[1];
}

// max over the aligned group of 8 consecutive lanes (every lane of the group gets it): group_sum's first three DPP steps
__device__ inline float group8_max(float v) {
  v = fmaxf(v, dpp_move<0xB1>(v));   // quad_perm(1,0,3,2)
  v = fmaxf(v, dpp_move<0x4E>(v));   // quad_perm(2,3,0,1)
  v = fmaxf(v, dpp_move<0x141>(v));  // row_half_mirror
  return v;
}
// max over the wave, every lane gets it (wave_sum_fast's ladder)
__device__ inline float wave_max_fast(float v) {
  v = group8_max(v);
  v = fmaxf(v, dpp_move<0x140>(v));  // row_mirror
  const int iv = __float_as_int(v);
  auto a = __builtin_amdgcn_permlane16_swap(iv, iv, false, false);
  v = fmaxf(__int_as_float(a[0]), __int_as_float(a[1]));
  const int iw = __float_as_int(v);
  auto b = __builtin_amdgcn_permlane32_swap(iw, iw, false, false);
  return fmaxf(__int_as_float(b[0]), __int_as_float(b[1]));
}
// sum over the aligned group of 4 consecutive lanes: group_sum's first two DPP steps
__device__ inline float group4_sum(float v) {
  v += dpp_move<0xB1>(v);  // quad_perm(1,0,3,2)
  v += dpp_move<0x4E>(v);  // quad_perm(2,3,0,1)
  return v;
}

// ---------------------------------------------------------------------------------------------------
// packed prefill store
// ---------------------------------------------------------------------------------------------------
// kv_store_seqs_kernel<bf16, true> with Q() between the load and the store.  One lane per 16 bytes of a K row and of a V row: the 8
// lanes of an (event, head) row are an aligned lane group, they take every drop decision together (the decisions depend on the
// row alone), and they reduce amax with three DPP moves.  Each lane writes 8 code bytes of K and of V; lane 0 of the group writes
// the scale pair.
__global__ __launch_bounds__(256) void kvq_store_seqs_kernel(const bf16* __restrict__ qkv, const int32_t* __restrict__ seq_start,
                                                             const int32_t* __restrict__ rows, uint8_t* __restrict__ k8,
                                                             uint8_t* __restrict__ v8, float* __restrict__ sc, int n, int64_t M,
                                                             int H, int64_t Lmax, int B) {
  constexpr int cph = QHD / 8;
  const int64_t total = M * H * cph;
  const int64_t D = (int64_t)H * QHD;
  const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (it >= total) return;
  const int c = (int)(it % cph);
  const int64_t r = it / cph;
  const int h = (int)(r % H);
  const int64_t m = r / H;
  int lo = 0, hi = n;  // seq_start[lo] <= m < seq_start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)seq_start[mid] <= m) lo = mid; else hi = mid;
  }
  const int64_t row = m - seq_start[lo];
  if (row < 0 || row >= Lmax) return;
  const int seq = rows[lo];
  if (seq < 0 || seq >= B) return;
  const bf16* src = qkv + m * 3 * D + (int64_t)h * QHD + c * 8;
  float kf[8], vf[8];
  expand8_bf16(ld16(src + D).v, kf);
  expand8_bf16(ld16(src + 2 * D).v, vf);
  float ka = 0.f, va = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    ka = fmaxf(ka, fabsf(kf[e]));
    va = fmaxf(va, fabsf(vf[e]));
  }
  const float ks = kvq_scale(group8_max(ka)), vs = kvq_scale(group8_max(va));
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    kf[e] = kvq_quot(kf[e], ks);
    vf[e] = kvq_quot(vf[e], vs);
  }
  const int64_t drow = ((int64_t)seq * H + h) * Lmax + row;
  const kvq_u32x2 kw = {kvq_pack4(kf[0], kf[1], kf[2], kf[3]), kvq_pack4(kf[4], kf[5], kf[6], kf[7])};
  const kvq_u32x2 vw = {kvq_pack4(vf[0], vf[1], vf[2], vf[3]), kvq_pack4(vf[4], vf[5], vf[6], vf[7])};
  *reinterpret_cast<kvq_u32x2*>(k8 + drow * QHD + c * 8) = kw;
  *reinterpret_cast<kvq_u32x2*>(v8 + drow * QHD + c * 8) = vw;
  if (c == 0) *reinterpret_cast<kvq_f32x2*>(sc + drow * 2) = kvq_f32x2{ks, vs};
}

// ---------------------------------------------------------------------------------------------------
// fork
// ---------------------------------------------------------------------------------------------------
// kv_fork_rows_kernel over the fp8 cache.  For a fixed (layer, sequence, head) the codes of positions [0, len) are len * 64
// contiguous bytes and the scales len * 8: blockIdx.x walks the run in chunks of 64 positions -- every lane copies 16 bytes of K
// codes and of V codes, and the first 64 lanes copy one position's scale pair each.  blockIdx.y = layer * H + head, blockIdx.z = the
// pair; the dropped-pair rules are the bf16 kernel's.
__global__ __launch_bounds__(256) void kvq_fork_rows_kernel(uint8_t* __restrict__ k8, uint8_t* __restrict__ v8,
                                                            float* __restrict__ sc, const int32_t* __restrict__ src,
                                                            const int32_t* __restrict__ dst, const int32_t* __restrict__ len,
                                                            int B, int H, int64_t Lmax) {
  const int p = blockIdx.z;
  const int s = src[p], d = dst[p];
  if (s < 0 || s >= B || d < 0 || d >= B || s == d) return;
  int64_t L = len[p];
  if (L > Lmax) L = Lmax;
  const int64_t layer = blockIdx.y / H, h = blockIdx.y % H;
  const int64_t from = ((layer * B + s) * H + h) * Lmax, to = ((layer * B + d) * H + h) * Lmax;  // in positions
  const int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;  // byte of the code run
  if (e < L * QHD) {
    // (src != dst: the runs are disjoint)
    *reinterpret_cast<kvq_u32x4*>(k8 + to * QHD + e) = *reinterpret_cast<const kvq_u32x4*>(k8 + from * QHD + e);
    *reinterpret_cast<kvq_u32x4*>(v8 + to * QHD + e) = *reinterpret_cast<const kvq_u32x4*>(v8 + from * QHD + e);
  }
  const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;  // position of the scale pair
  if (threadIdx.x < 64 && j < L)
    *reinterpret_cast<kvq_u32x2*>(sc + (to + j) * 2) = *reinterpret_cast<const kvq_u32x2*>(sc + (from + j) * 2);
}

// ---------------------------------------------------------------------------------------------------
// decode attention, per-row positions, append fused
// ---------------------------------------------------------------------------------------------------
// attn_decode_kernel<bf16, 64, APPEND, false, ROWS> over the fp8 cache: one block (4 waves) per (head, sequence), grid (H, B), the
// position from row_pos[b].  A key row is 64 code bytes: LPK = 4 lanes with 16-byte loads, 16 elements of q and of the accumulator
// per lane, 16 keys per wave and round.  (8 bytes per lane would keep the bf16 kernel's 8 lanes per key and its 8-element
// accumulators, at twice the load instructions per byte; the 16-byte form was taken because the load count per key is what the
// bf16 kernel's key loop is built around.)  The loop has that kernel's shape: UNR rounds per step, two register sets, the next
// step's loads issued before the current step's arithmetic behind a sched_barrier, the per-key sum on DPP moves, out-of-range
// keys masked.  The arithmetic per key j (ks_j, vs_j its scale pair):
//   score_j = (sum_e q_e * float(kcode_je)) * ks_j;      acc_e = acc_e * a + (p_j * vs_j) * float(vcode_je)
// -- one multiply per key for each scale.
// The new position: wave 0 rotates k, rounds it to bf16 as attn_decode_kernel does, computes Q() of the k row and of the v row
// (amax over the wave on DPP / permlane moves), stores codes and the scale pair to the cache and to LDS; the block attends to
// that row from LDS, dequantized -- "as the cache holds it".
template <int UNR>
__global__ __launch_bounds__(256) void kvq_attn_decode_kernel(const bf16* __restrict__ qkv, uint8_t* k8, uint8_t* v8, float* sc,
                                                              bf16* __restrict__ o, int H, int64_t Lmax, float scale,
                                                              const int32_t* __restrict__ row_pos,
                                                              const float* __restrict__ cos_t, const float* __restrict__ sin_t) {
  // every kernel argument fetched at entry in one batch (attn_decode_kernel has the reason)
  asm volatile("" ::"s"(qkv), "s"(k8), "s"(v8), "s"(sc), "s"(o), "s"(H), "s"(Lmax), "s"(scale));
  asm volatile("" ::"s"(row_pos), "s"(cos_t), "s"(sin_t));
  int64_t len = (int64_t)row_pos[blockIdx.y] + 1;  // this sequence's position
  if (len < 1) len = 1;
  if (len > Lmax) len = Lmax;
  constexpr int HD = QHD, half = HD / 2;
  constexpr int N = 16;             // elements per lane
  constexpr int LPK = HD / N;       // lanes per key row
  constexpr int KPW = 64 / LPK;     // keys per wave per round
  __shared__ float sh_m[4], sh_l[4];
  __shared__ float sh_o[4][HD];
  __shared__ __attribute__((aligned(16))) uint8_t sh_kn[HD], sh_vn[HD];  // the new row's codes ...
  __shared__ float sh_sn[2];                                              // ... and its scale pair
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t b = blockIdx.y;
  const int h = blockIdx.x;
  const int64_t bh = b * H + h;
  const int64_t D = (int64_t)H * HD;
  const int ch = lane % LPK, grp = lane / LPK;
  const bf16* qrow = qkv + b * 3 * D + (int64_t)h * HD;
  const int64_t pos = len - 1;
  if (wv == 0) {  // k row (rotated, rounded to bf16) and v row of the new position -> Q() -> cache and LDS
    const int i = lane & 31;  // (lanes 32 to 63 repeat lanes 0 to 31, so that the wave-wide max is the row's; they store nothing)
    const float c = rnd<bf16>(cos_t[pos * half + i]), sn = rnd<bf16>(sin_t[pos * half + i]);
    const float k1 = to_f(qrow[D + i]), k2 = to_f(qrow[D + i + half]);
    const float ka = rnd<bf16>(k1 * c - k2 * sn), kb2 = rnd<bf16>(k2 * c + k1 * sn);
    const float va = to_f(qrow[2 * D + i]), vb2 = to_f(qrow[2 * D + i + half]);
    const float ks = kvq_scale(wave_max_fast(fmaxf(fabsf(ka), fabsf(kb2))));
    const float vs = kvq_scale(wave_max_fast(fmaxf(fabsf(va), fabsf(vb2))));
    const unsigned kw = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(kvq_quot(ka, ks), kvq_quot(kb2, ks), 0, false);
    const unsigned vw = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(kvq_quot(va, vs), kvq_quot(vb2, vs), 0, false);
    if (lane < half) {
      uint8_t* kd = k8 + (bh * Lmax + pos) * HD;
      uint8_t* vd = v8 + (bh * Lmax + pos) * HD;
      const uint8_t c0 = (uint8_t)(kw & 0xff), c1 = (uint8_t)((kw >> 8) & 0xff);
      const uint8_t d0 = (uint8_t)(vw & 0xff), d1 = (uint8_t)((vw >> 8) & 0xff);
      kd[i] = c0;
      kd[i + half] = c1;
      vd[i] = d0;
      vd[i + half] = d1;
      sh_kn[i] = c0;
      sh_kn[i + half] = c1;
      sh_vn[i] = d0;
      sh_vn[i + half] = d1;
      if (lane == 0) {
        *reinterpret_cast<kvq_f32x2*>(sc + (bh * Lmax + pos) * 2) = kvq_f32x2{ks, vs};
        sh_sn[0] = ks;
        sh_sn[1] = vs;
      }
    }
  }
  float q[N];
  {
    const int base = ch * N;  // this lane's q elements and their rotation partners (i, i + half)
    float qf[N], qp[N];
    {
      float t0[8], t1[8];
      expand8_bf16(ld16(qrow + base).v, t0);
      expand8_bf16(ld16(qrow + base + 8).v, t1);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        qf[e] = t0[e];
        qf[e + 8] = t1[e];
      }
      const int pb = (base + half) % HD;
      expand8_bf16(ld16(qrow + pb).v, t0);
      expand8_bf16(ld16(qrow + pb + 8).v, t1);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        qp[e] = t0[e];
        qp[e + 8] = t1[e];
      }
    }
#pragma unroll
    for (int e = 0; e < N; ++e) {
      const int i = (base + e) % half;
      const float c = rnd<bf16>(cos_t[pos * half + i]), sn = rnd<bf16>(sin_t[pos * half + i]);
      const float r = (base < half) ? qf[e] * c - qp[e] * sn : qf[e] * c + qp[e] * sn;
      q[e] = rnd<bf16>(r) * scale;
    }
  }
  __syncthreads();  // the new row's codes and scales are visible to the whole block
  float m = -INFINITY, l = 0.f, acc[N];
#pragma unroll
  for (int e = 0; e < N; ++e) acc[e] = 0.f;
  const uint8_t* kb = k8 + bh * Lmax * HD;
  const uint8_t* vb = v8 + bh * Lmax * HD;
  const float* sb = sc + bh * Lmax * 2;
  constexpr int STEP = 4 * KPW * UNR;
  const int ilen = (int)len - 1;  // the rows read from the cache (<= Lmax < 2^24: 32-bit offsets); the new one comes from LDS below
  const int lane_off = ch * N;
  kvq_u32x4 kvA[UNR], vvA[UNR], kvB[UNR], vvB[UNR];
  kvq_f32x2 scA[UNR], scB[UNR];
  bool okA[UNR], okB[UNR];
  auto request = [&](kvq_u32x4 (&kv)[UNR], kvq_u32x4 (&vv)[UNR], kvq_f32x2 (&ss)[UNR], bool (&ok)[UNR], int j0) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = j0 + u * 4 * KPW + grp;
      ok[u] = j < ilen;
      const unsigned jj = (unsigned)(ok[u] ? j : 0);
      kv[u] = *reinterpret_cast<const kvq_u32x4*>(kb + jj * HD + lane_off);
      vv[u] = *reinterpret_cast<const kvq_u32x4*>(vb + jj * HD + lane_off);
      ss[u] = *reinterpret_cast<const kvq_f32x2*>(sb + jj * 2);
    }
  };
  // one key: the codes of its K and V rows (this lane's 16 bytes of each), its scale pair, and whether it counts
  auto key = [&](const kvq_u32x4& kw, const kvq_u32x4& vw, const kvq_f32x2& ss, bool ok) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      float f[4];
      kvq_unpack4(kw[w], f);
#pragma unroll
      for (int e = 0; e < 4; ++e) s += q[4 * w + e] * f[e];
    }
    s = group4_sum(s) * ss[0];
    if (ok) {
      const float nm = fmaxf(m, s);
      const float a = __expf(m - nm), p = __expf(s - nm);
      l = l * a + p;
      const float pv = p * ss[1];
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        float f[4];
        kvq_unpack4(vw[w], f);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * w + e] = acc[4 * w + e] * a + pv * f[e];
      }
      m = nm;
    }
  };
  auto reduce = [&](const kvq_u32x4 (&kv)[UNR], const kvq_u32x4 (&vv)[UNR], const kvq_f32x2 (&ss)[UNR], const bool (&ok)[UNR]) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) key(kv[u], vv[u], ss[u], ok[u]);
  };
  int j0 = wv * KPW;
  if (j0 < ilen) {
    request(kvA, vvA, scA, okA, j0);
    while (true) {
      const int j1 = j0 + STEP;
      if (j1 < ilen) request(kvB, vvB, scB, okB, j1);
      // (the requests above are issued before the first dot product below: attn_decode_kernel has the reason)
      __builtin_amdgcn_sched_barrier(0);
      reduce(kvA, vvA, scA, okA);
      if (j1 >= ilen) break;
      j0 = j1 + STEP;
      if (j0 < ilen) request(kvA, vvA, scA, okA, j0);
      __builtin_amdgcn_sched_barrier(0);
      reduce(kvB, vvB, scB, okB);
      if (j0 >= ilen) break;
    }
  }
  if (wv == 0) {  // the new position's key / value, dequantized from LDS: lane group 0 of wave 0
    const kvq_u32x4 kn = *reinterpret_cast<const kvq_u32x4*>(sh_kn + lane_off);
    const kvq_u32x4 vn = *reinterpret_cast<const kvq_u32x4*>(sh_vn + lane_off);
    key(kn, vn, kvq_f32x2{sh_sn[0], sh_sn[1]}, grp == 0);
  }
  // merge the KPW lane groups of the wave (lanes with equal `ch`)
#pragma unroll
  for (int x = LPK; x < 64; x <<= 1) {
    const float om = __shfl_xor(m, x, 64), ol = __shfl_xor(l, x, 64);
    const float nm = fmaxf(m, om);
    const float a = (m == -INFINITY) ? 0.f : __expf(m - nm);
    const float bsc = (om == -INFINITY) ? 0.f : __expf(om - nm);
    l = l * a + ol * bsc;
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = acc[e] * a + __shfl_xor(acc[e], x, 64) * bsc;
    m = nm;
  }
  if (lane < LPK) {
#pragma unroll
    for (int e = 0; e < N; ++e) sh_o[wv][ch * N + e] = acc[e];
    if (lane == 0) {
      sh_m[wv] = m;
      sh_l[wv] = l;
    }
  }
  __syncthreads();
  if (threadIdx.x < HD) {
    const float gm = fmaxf(fmaxf(sh_m[0], sh_m[1]), fmaxf(sh_m[2], sh_m[3]));
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float f = (sh_m[w] == -INFINITY) ? 0.f : __expf(sh_m[w] - gm);
      num += sh_o[w][threadIdx.x] * f;
      den += sh_l[w] * f;
    }
    o[b * D + (int64_t)h * HD + threadIdx.x] = from_f<bf16>(num / den);
  }
}

}  // namespace

// rounds per step of the decode kernel's key loop (4 waves x 16 keys x UNR keys per register set)
#define MH_KVQ_UNR 4

extern "C" int mh_kv_store_seqs_rows_fp8(const void* qkv, const int32_t* seq_start, const int32_t* rows, void* k8, void* v8,
                                         float* sc, int64_t n, int64_t B, int64_t M, int H, int hd, int64_t Lmax, int dtype,
                                         void* stream) {
  MH_REQUIRE(qkv != nullptr && seq_start != nullptr && k8 != nullptr && v8 != nullptr && sc != nullptr,
             "kv_store_seqs_rows_fp8: null buffer");
  MH_REQUIRE(rows != nullptr, "kv_store_seqs_rows_fp8: rows is NULL (one device int32 cache row per sequence)");
  MH_REQUIRE(dtype == MH_BF16, "kv_store_seqs_rows_fp8: dtype %d (the fp8 cache takes bf16 activations)", dtype);
  MH_REQUIRE(hd == QHD, "kv_store_seqs_rows_fp8: head_dim %d unsupported (64)", hd);
  MH_REQUIRE(n > 0 && B > 0 && B < (1 << 30) && M >= n && M < (1ll << 31) && H > 0 && Lmax > 0,
             "kv_store_seqs_rows_fp8: bad args n=%ld B=%ld M=%ld H=%d Lmax=%ld", (long)n, (long)B, (long)M, H, (long)Lmax);
  MH_REQUIRE(n <= B, "kv_store_seqs_rows_fp8: %ld sequences for a cache of %ld", (long)n, (long)B);
  MH_REQUIRE(M <= n * Lmax, "kv_store_seqs_rows_fp8: %ld rows in %ld sequences: a length exceeds Lmax=%ld", (long)M, (long)n,
             (long)Lmax);
  const int64_t total = M * H * (QHD / 8);
  const int64_t g = (total + 255) / 256;
  MH_REQUIRE(g < (1ll << 31), "kv_store_seqs_rows_fp8: %ld workgroups", (long)g);
  kvq_store_seqs_kernel<<<(unsigned)g, 256, 0, (hipStream_t)stream>>>((const bf16*)qkv, seq_start, rows, (uint8_t*)k8, (uint8_t*)v8,
                                                                      sc, (int)n, M, H, Lmax, (int)B);
  MH_LAUNCH_CHECK();
  return MH_OK;
}

extern "C" int mh_attn_decode_append_rows_fp8(const void* qkv, const float* cos_t, const float* sin_t, void* k8, void* v8,
                                              float* sc, void* o, int64_t B, int H, int hd, int64_t Lmax, float scale,
                                              const int32_t* row_pos, int dtype, void* stream) {
  MH_REQUIRE(hd == QHD, "attn_decode_append_rows_fp8: head_dim %d unsupported (64)", hd);
  MH_REQUIRE(dtype == MH_BF16, "attn_decode_append_rows_fp8: dtype %d (the fp8 cache takes bf16 activations)", dtype);
  MH_REQUIRE(row_pos != nullptr, "attn_decode_append_rows_fp8: row_pos is NULL (one device int32 position per sequence)");
  MH_REQUIRE(B > 0 && B < 65536 && H > 0 && Lmax > 0 && Lmax < (1 << 24), "attn_decode_append_rows_fp8: bad args B=%ld H=%d Lmax=%ld",
             (long)B, H, (long)Lmax);
  MH_REQUIRE(qkv != nullptr && cos_t != nullptr && sin_t != nullptr && k8 != nullptr && v8 != nullptr && sc != nullptr &&
                 o != nullptr, "attn_decode_append_rows_fp8: null buffer (the rope tables are needed: qkv arrives unrotated)");
  const dim3 grid((unsigned)H, (unsigned)B);
  kvq_attn_decode_kernel<MH_KVQ_UNR><<<grid, 256, 0, (hipStream_t)stream>>>((const bf16*)qkv, (uint8_t*)k8, (uint8_t*)v8, sc,
                                                                            (bf16*)o, H, Lmax, scale, row_pos, cos_t, sin_t);
  MH_LAUNCH_CHECK();
  return MH_OK;
}

extern "C" int mh_kv_fork_rows_fp8(void* k8, void* v8, float* sc, const int32_t* src, const int32_t* dst, const int32_t* len,
                                   int64_t n, int64_t max_len, int64_t layers, int64_t B, int H, int hd, int64_t Lmax,
                                   void* stream) {
  MH_REQUIRE(k8 != nullptr, "kv_fork_rows_fp8: k8 is NULL");
  MH_REQUIRE(v8 != nullptr, "kv_fork_rows_fp8: v8 is NULL");
  MH_REQUIRE(sc != nullptr, "kv_fork_rows_fp8: sc is NULL");
  MH_REQUIRE(src != nullptr, "kv_fork_rows_fp8: src is NULL (one device int32 cache row per pair)");
  MH_REQUIRE(dst != nullptr, "kv_fork_rows_fp8: dst is NULL (one device int32 cache row per pair)");
  MH_REQUIRE(len != nullptr, "kv_fork_rows_fp8: len is NULL (one device int32 length per pair)");
  MH_REQUIRE(hd == QHD, "kv_fork_rows_fp8: head_dim %d unsupported (64)", hd);
  MH_REQUIRE(layers > 0 && B > 0 && B < (1 << 30) && H > 0 && Lmax > 0 && Lmax < (1ll << 31),
             "kv_fork_rows_fp8: bad args layers=%ld B=%ld H=%d Lmax=%ld", (long)layers, (long)B, H, (long)Lmax);
  MH_REQUIRE(n >= 1 && n <= B, "kv_fork_rows_fp8: %ld pairs for a cache of %ld sequences", (long)n, (long)B);
  MH_REQUIRE(max_len >= 1 && max_len <= Lmax, "kv_fork_rows_fp8: max_len %ld outside [1, Lmax=%ld]", (long)max_len, (long)Lmax);
  const int64_t gx = (max_len + 63) / 64, gy = layers * H;  // a workgroup covers 64 positions of a run
  MH_REQUIRE(gx < (1ll << 31) && gy <= 65535 && n <= 65535, "kv_fork_rows_fp8: a grid of %ld x %ld x %ld workgroups", (long)gx,
             (long)gy, (long)n);
  kvq_fork_rows_kernel<<<dim3((unsigned)gx, (unsigned)gy, (unsigned)n), 256, 0, (hipStream_t)stream>>>(
      (uint8_t*)k8, (uint8_t*)v8, sc, src, dst, len, (int)B, H, Lmax);
  MH_LAUNCH_CHECK();
  return MH_OK;
}
