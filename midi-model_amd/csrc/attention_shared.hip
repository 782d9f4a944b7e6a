// Decode attention over a prompt that all B rows of the batch share (generate(share_prompt=True)): the prefix half.
//
// The prompt's K/V live ONCE, as [H, Pmax, 64] per layer, and every decoded event reads them once per head for all B rows:
//   mh_attn_prefix_partial        (this file)   a workgroup owns one head and one chunk of PREFIX_CHUNK prefix keys, rotates the
//                                               B query rows of its head, and leaves per (b, h, chunk) an UNNORMALISED fp32
//                                               acc[64] plus the chunk's running maximum m and sum l in a workspace
//   mh_attn_decode_append_shared  (attention_small.hip: attn_decode_kernel<.., SHARED>) the row's own suffix cache, then the
//                                               merge of its ceil(pre_len / PREFIX_CHUNK) partials in chunk order, then 1 / l
// Two launches with a fixed order of additions: the same bits on every run.
//
// PREFIX_CHUNK = 256.  The grid is H x ceil(Pmax / 256) whatever pre_len is (a captured graph serves every prompt length): 16
// heads x 16 chunks = 256 workgroups at the serving loop's 4096-event crop, one per CU of an MI355X, each streaming 64 KiB of
// K/V.  128 would double the partials (B x H x chunks x 264 bytes written and read back per layer: 8.6 MB at B = 64, half of the
// 16.8 MB of K/V the launch exists to read once) for workgroups the device has no second CU for; 512 leaves half the CUs idle
// at 4096 and all but H x 2 at 1024.  Chunks at or past ceil(pre_len / 256) return at once and write nothing.
//
// bf16 form, orientation of the flash forward (attention_mfma.hip): S^T = K Q^T, O^T += V^T P^T with the QUERY ROW on the lane
// axis (v_mfma_f32_32x32x16_bf16: 32 rows of the batch per pass, padded by repeating the last row), so the softmax state is
// lane-local and P goes from the accumulator to the next MFMA's operand in registers.  Wave w owns keys [64 w, 64 w + 64) of
// the chunk: it stages its own K and V tiles (row-major, the swizzled format of common.h), takes the K fragments with
// ds_read_b128 and the V^T fragments with ds_read_b64_tr_b16 (tr_frag_offsets) ONCE, and runs every 32-row tile of the batch
// against them from registers.  The four waves' states meet in LDS and leave as one partial.  P is rounded to bf16 for the P V
// product as in the event forward; m, l and acc are fp32.
// fp32 form: plain VALU, one workgroup per (head, chunk, row); it exists for the parity tests, not for speed.
//
// SLOTS (mh_attn_prefix_partial_slots; DecodeSession(prefix_slots=G), the decode pool): G prompts, kpre / vpre [G, H, Pmax, 64],
// and every row of the batch at a position of its own.  slot_len [G] (0: an empty slot), row_slot [B] (-1, or any value outside
// [0, G): the row shares nothing) and row_pos [B] are device int32 arrays.  The grid gains a dimension -- blockIdx.y is the slot --
// and a workgroup serves the MEMBER rows of its slot only: every wave walks row_slot 64 rows at a time, a ballot per step, and
// wave 0 leaves the members' row ids in LDS in ascending order (behind the merge area; 4 B bytes).  The tiles of 32 query rows are
// then tiles of that list, each lane's row rotated at its own row_pos, and a partial goes to the workspace index of its ROW,
// ((b H + h) nch + c), so the consumer's addressing is the uniform form's.  A slot without members, like a chunk past the slot's
// length, returns at once.  One body serves both forms (`if constexpr`): per query row the arithmetic and its order are the same,
// and an MFMA output column depends on its own query column alone, so a member row's partial is bit for bit the uniform
// kernel's for that row at that (pre_len, pos), whatever else shares its tile.
#include "attn_mfma_common.h"

constexpr int PREFIX_CHUNK = MH_ATTN_PREFIX_CHUNK;
constexpr int PP_TILES = 4 * 2 * TILE64;             // [wave][K | V] tiles
constexpr int PP_MERGE_ACC = 4 * 64 * 32 * 4;        // [wave][d][row] fp32 (row fastest: lane-consecutive, no bank conflicts)
constexpr int PP_MERGE_ML = 4 * 2 * 32 * 4;          // [wave][m | l][row]
constexpr int PP_LDS = PP_TILES + PP_MERGE_ACC + PP_MERGE_ML;
constexpr int PP_MAX_ROWS = 4096;                    // (slots form) rows of a batch: the member list, 4 bytes a row behind PP_LDS

// workspace: acc [B, H, nch, 64] followed by (m, l) [B, H, nch, 2]; nch = ceil(Pmax / PREFIX_CHUNK)
__host__ __device__ inline int64_t prefix_ws_floats(int64_t B, int H, int nch) { return B * H * nch * 66; }

// SLOTS: pre_len_dev is slot_len [G], pos_dev is row_pos [B], row_slot [B] names each row's slot (the host values are not read)
template <bool SLOTS>
__global__ __launch_bounds__(256) void attn_prefix_partial_mfma_kernel(
    const bf16* __restrict__ qkv, const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    const bf16* __restrict__ kpre, const bf16* __restrict__ vpre, float* __restrict__ ws, int B, int H, int Pmax, int nch,
    int pre_len, int pos, float scale, const int32_t* __restrict__ pre_len_dev, const int32_t* __restrict__ pos_dev,
    const int32_t* __restrict__ row_slot) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if constexpr (SLOTS) {
    pre_len = pre_len_dev[blockIdx.y];
  } else {
    if (pre_len_dev != nullptr) pre_len = *pre_len_dev;  // graph replay: both live in device memory
    if (pos_dev != nullptr) pos = *pos_dev;
  }
  if (pre_len > Pmax) pre_len = Pmax;
  const int h = blockIdx.x / nch, c = blockIdx.x - h * nch;
  const int k0 = c * PREFIX_CHUNK;
  if (k0 >= pre_len) return;  // (block-uniform) nothing of the prompt in this chunk: no partial, and none is read
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int nrow = B;  // the query rows this workgroup serves
  int32_t* members = reinterpret_cast<int32_t*>(smem + PP_LDS);  // (SLOTS) their row ids, ascending
  if constexpr (SLOTS) {
    const int g = blockIdx.y;
    nrow = 0;  // (wave-uniform, and the same in all four waves: each walks the whole of row_slot)
    for (int b0 = 0; b0 < B; b0 += 64) {
      const int b = b0 + lane;
      const bool in = b < B && row_slot[b] == g;
      const unsigned long long bal = __ballot(in);
      if (in && wave == 0) members[nrow + __popcll(bal & ((1ull << lane) - 1ull))] = b;
      nrow += __popcll(bal);
    }
    if (nrow == 0) return;  // (block-uniform) no row continues this slot's prompt
    kpre += (int64_t)g * H * Pmax * HD;
    vpre += (int64_t)g * H * Pmax * HD;
  }
  const int kw0 = k0 + 64 * wave;
  const bool live = kw0 < pre_len;  // (wave-uniform) key kw0 is then a real one: every row's maximum is finite
  char* tK = smem + wave * 2 * TILE64;
  char* tV = tK + TILE64;
  if (live) {
    const bf16* kb = kpre + (int64_t)h * Pmax * HD;
    const bf16* vb = vpre + (int64_t)h * Pmax * HD;
    const int rsub = lane >> 3, ch = lane & 7;
    bf16x8 kr[8], vr[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) {  // rows past the prompt repeat its last row (never the poison behind it); masked below
      int g = kw0 + it * 8 + rsub;
      g = g < pre_len ? g : pre_len - 1;
      const int64_t off = (int64_t)g * HD + ch * 8;
      kr[it] = *reinterpret_cast<const bf16x8*>(kb + off);
      vr[it] = *reinterpret_cast<const bf16x8*>(vb + off);
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int r = it * 8 + rsub;
      *reinterpret_cast<bf16x8*>(tK + lds_tile_off(r, ch)) = kr[it];
      *reinterpret_cast<bf16x8*>(tV + lds_tile_off(r, ch)) = vr[it];
    }
  }
  __syncthreads();
  const int li = lane & 31, hi = lane >> 5, pli = pi32(li);
  bf16x8 kf[2][4];
  u32x2 vt[4][2][2];  // [16-key step][32-wide half of d][half of the 8-deep fragment]
  if (live) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int s = 0; s < 4; ++s) kf[kb][s] = lds_frag(tK, kb * 32 + pli, 2 * s + hi);
    int trof[2][2];
    tr_frag_offsets(lane, trof);
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const unsigned a = lds_addr32(tV) + (unsigned)trof[db][half];
        vt[0][db][half] = ds_tr16<0>(a);
        vt[1][db][half] = ds_tr16<2048>(a);
        vt[2][db][half] = ds_tr16<4096>(a);
        vt[3][db][half] = ds_tr16<6144>(a);
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the transpose reads (asm: invisible to hipcc's counters)
    __builtin_amdgcn_sched_barrier(0);
  }
  float* mg_acc = reinterpret_cast<float*>(smem + PP_TILES);
  float* mg_ml = reinterpret_cast<float*>(smem + PP_TILES + PP_MERGE_ACC);
  const int64_t D = (int64_t)H * HD;
  float* ws_ml = ws + (int64_t)B * H * nch * 64;
  const int nqt = (nrow + 31) / 32;
  for (int qt = 0; qt < nqt; ++qt) {
    if (live) {
      int bq = qt * 32 + li;
      bq = bq < nrow ? bq : nrow - 1;
      if constexpr (SLOTS) {  // (the list was written before the barrier above)
        bq = members[bq];
        pos = pos_dev[bq];
        pos = pos > 0 ? pos : 0;
      }
      const bf16* qp = qkv + (int64_t)bq * 3 * D + (int64_t)h * HD + 8 * hi;
      bf16x8 raw[4], qf[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) raw[s] = *reinterpret_cast<const bf16x8*>(qp + 16 * s);
      // q rotated at `pos` as kv_append does it (cos / sin rounded to bf16, the result rounded to bf16), then x scale
      // (exact for the power of two 1/8; the lane holds both partners d and d + 32 of a pair: fragments s and s + 2)
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int i = 16 * s + 8 * hi + e;
          const float cs = rnd<bf16>(cos_t[(int64_t)pos * 32 + i]), sn = rnd<bf16>(sin_t[(int64_t)pos * 32 + i]);
          const float x1 = (float)raw[s][e], x2 = (float)raw[s + 2][e];
          qf[s][e] = (bf16)(rnd<bf16>(x1 * cs - x2 * sn) * scale);
          qf[s + 2][e] = (bf16)(rnd<bf16>(x2 * cs + x1 * sn) * scale);
        }
      f32x16 sacc[2] = {zero16(), zero16()};
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) sacc[kb] = mfma32(kf[kb][s], qf[s], sacc[kb]);
      float mx = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (kw0 + kb * 32 + reg_index(r, hi) >= pre_len) sacc[kb][r] = -INFINITY;
          mx = fmaxf(mx, sacc[kb][r]);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mx2 = mx * LOG2E;
      float psum = 0.f;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = fast_exp2(__builtin_fmaf(sacc[kb][r], LOG2E, -mx2));
          sacc[kb][r] = p;
          psum += p;
        }
      const float l = psum + __shfl_xor(psum, 32, 64);
      f32x16 oacc[2] = {zero16(), zero16()};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const bf16x8 pf = pack8(sacc[t >> 1], 8 * (t & 1));
#pragma unroll
        for (int db = 0; db < 2; ++db) oacc[db] = mfma32(join8(vt[t][db][0], vt[t][db][1]), pf, oacc[db]);
      }
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) mg_acc[(wave * 64 + db * 32 + reg_index(r, hi)) * 32 + li] = oacc[db][r];
      if (hi == 0) {
        mg_ml[(wave * 2) * 32 + li] = mx;
        mg_ml[(wave * 2 + 1) * 32 + li] = l;
      }
    } else if (lane < 32) {
      mg_ml[(wave * 2) * 32 + lane] = -INFINITY;
      mg_ml[(wave * 2 + 1) * 32 + lane] = 0.f;
    }
    __syncthreads();
    {  // the four waves' states -> one partial per row: thread = (row q, eight consecutive d)
      const int q = tid & 31, dg = tid >> 5;
      int bq = qt * 32 + q;
      const bool real = bq < nrow;  // (not a padding row of the last tile)
      if constexpr (SLOTS) bq = members[real ? bq : 0];
      float mw[4], f[4], gm = -INFINITY, lsum = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        mw[w] = mg_ml[(w * 2) * 32 + q];
        gm = fmaxf(gm, mw[w]);
      }
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        f[w] = (mw[w] == -INFINITY) ? 0.f : fast_exp2((mw[w] - gm) * LOG2E);
        lsum += mg_ml[(w * 2 + 1) * 32 + q] * f[w];
      }
      if (real) {
        float out[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float a = 0.f;
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const float v = mg_acc[(w * 64 + dg * 8 + j) * 32 + q];
            a += (mw[w] == -INFINITY) ? 0.f : v * f[w];  // (a wave without keys wrote no acc)
          }
          out[j] = a;
        }
        const int64_t idx = ((int64_t)bq * H + h) * nch + c;
        float* dst = ws + idx * 64 + dg * 8;
        *reinterpret_cast<f32x4*>(dst) = f32x4{out[0], out[1], out[2], out[3]};
        *reinterpret_cast<f32x4*>(dst + 4) = f32x4{out[4], out[5], out[6], out[7]};
        if (dg == 0) {
          ws_ml[idx * 2] = gm;
          ws_ml[idx * 2 + 1] = lsum;
        }
      }
    }
    __syncthreads();  // the merge area is rewritten by the next tile of rows
  }
}

// fp32 (parity) form: grid (H * nch, B), thread = key of the chunk.
// SLOTS: the arguments as in the MFMA form; the row looks its own slot up (G slots), and a row without one returns at once.
template <typename T, bool SLOTS = false>
__global__ __launch_bounds__(256) void attn_prefix_partial_valu_kernel(
    const T* __restrict__ qkv, const float* __restrict__ cos_t, const float* __restrict__ sin_t, const T* __restrict__ kpre,
    const T* __restrict__ vpre, float* __restrict__ ws, int B, int H, int Pmax, int nch, int pre_len, int pos, float scale,
    const int32_t* __restrict__ pre_len_dev, const int32_t* __restrict__ pos_dev, const int32_t* __restrict__ row_slot = nullptr,
    int G = 0) {
  if constexpr (SLOTS) {
    const int g = row_slot[blockIdx.y];
    if (g < 0 || g >= G) return;
    pre_len = pre_len_dev[g];
    pos = pos_dev[blockIdx.y];
    pos = pos > 0 ? pos : 0;
    kpre += (int64_t)g * H * Pmax * 64;
    vpre += (int64_t)g * H * Pmax * 64;
  } else {
    if (pre_len_dev != nullptr) pre_len = *pre_len_dev;
    if (pos_dev != nullptr) pos = *pos_dev;
  }
  if (pre_len > Pmax) pre_len = Pmax;
  const int h = blockIdx.x / nch, c = blockIdx.x - h * nch, b = blockIdx.y;
  const int k0 = c * PREFIX_CHUNK;
  if (k0 >= pre_len) return;
  __shared__ float sh_q[64], sh_p[PREFIX_CHUNK], sh_red[8];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t D = (int64_t)H * 64;
  if (tid < 32) {
    const T* qrow = qkv + (int64_t)b * 3 * D + (int64_t)h * 64;
    const float cs = rnd<T>(cos_t[(int64_t)pos * 32 + tid]), sn = rnd<T>(sin_t[(int64_t)pos * 32 + tid]);
    const float x1 = to_f(qrow[tid]), x2 = to_f(qrow[tid + 32]);
    sh_q[tid] = rnd<T>(x1 * cs - x2 * sn) * scale;
    sh_q[tid + 32] = rnd<T>(x2 * cs + x1 * sn) * scale;
  }
  __syncthreads();
  const int j = k0 + tid;
  const bool valid = j < pre_len;
  float s = -INFINITY;
  if (valid) {
    const T* krow = kpre + ((int64_t)h * Pmax + j) * 64;
    s = 0.f;
    for (int d = 0; d < 64; ++d) s += sh_q[d] * to_f(krow[d]);
  }
  const float wm = wave_max(s);
  if (lane == 0) sh_red[wv] = wm;
  __syncthreads();
  const float m = fmaxf(fmaxf(sh_red[0], sh_red[1]), fmaxf(sh_red[2], sh_red[3]));  // key k0 is valid: finite
  const float p = valid ? __expf(s - m) : 0.f;
  sh_p[tid] = p;
  const float wl = wave_sum(p);
  if (lane == 0) sh_red[4 + wv] = wl;
  __syncthreads();
  if (tid < 64) {
    const int n = (pre_len - k0) < PREFIX_CHUNK ? (pre_len - k0) : PREFIX_CHUNK;
    const T* vcol = vpre + ((int64_t)h * Pmax + k0) * 64 + tid;
    float a = 0.f;
    for (int jj = 0; jj < n; ++jj) a += sh_p[jj] * to_f(vcol[(int64_t)jj * 64]);
    const int64_t idx = ((int64_t)b * H + h) * nch + c;
    ws[idx * 64 + tid] = a;
    if (tid == 0) {
      float* ws_ml = ws + (int64_t)B * H * nch * 64;
      ws_ml[idx * 2] = m;
      ws_ml[idx * 2 + 1] = (sh_red[4] + sh_red[5]) + (sh_red[6] + sh_red[7]);
    }
  }
}

extern "C" int mh_attn_prefix_chunk(void) { return PREFIX_CHUNK; }

extern "C" int mh_attn_prefix_partial(const void* qkv, const float* cos_t, const float* sin_t, const void* kpre,
                                      const void* vpre, float* ws, int64_t ws_floats, int64_t B, int H, int hd, int64_t Pmax,
                                      int64_t pre_len, int64_t pos, float scale, const int32_t* pre_len_dev,
                                      const int32_t* pos_dev, int dtype, void* stream) {
  MH_REQUIRE(hd == 64, "attn_prefix_partial: head_dim %d unsupported (64)", hd);
  MH_REQUIRE(dtype == MH_BF16 || dtype == MH_F32, "attn_prefix_partial: bad dtype %d", dtype);
  MH_REQUIRE(qkv != nullptr && cos_t != nullptr && sin_t != nullptr && kpre != nullptr && vpre != nullptr && ws != nullptr,
             "attn_prefix_partial: null buffer (the rope tables are needed: qkv arrives unrotated)");
  MH_REQUIRE(B > 0 && B <= 65535 && H > 0 && Pmax > 0 && Pmax < (1 << 24), "attn_prefix_partial: bad args B=%ld H=%d Pmax=%ld",
             (long)B, H, (long)Pmax);
  MH_REQUIRE(pre_len_dev != nullptr || (pre_len >= 1 && pre_len <= Pmax), "attn_prefix_partial: bad args pre_len=%ld Pmax=%ld",
             (long)pre_len, (long)Pmax);
  MH_REQUIRE(pos_dev != nullptr || pos >= 0, "attn_prefix_partial: bad args pos=%ld", (long)pos);
  MH_REQUIRE(pre_len_dev != nullptr || pos_dev != nullptr || pos >= pre_len, "attn_prefix_partial: bad args pos=%ld < pre_len=%ld",
             (long)pos, (long)pre_len);
  const int nch = (int)((Pmax + PREFIX_CHUNK - 1) / PREFIX_CHUNK);
  MH_REQUIRE(ws_floats >= prefix_ws_floats(B, H, nch), "attn_prefix_partial: workspace of %ld floats, %ld needed",
             (long)ws_floats, (long)prefix_ws_floats(B, H, nch));
  MH_REQUIRE((int64_t)H * nch < (1 << 30), "attn_prefix_partial: grid too large");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MH_BF16) {
    constexpr int MAX_DEV = 64;
    static bool attr_set_of[MAX_DEV];
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) {
      mh_set_error("attn_prefix_partial: no current device (or ordinal %d beyond %d)", dev, MAX_DEV - 1);
      return MH_ERR_LAUNCH;
    }
    if (!__atomic_load_n(&attr_set_of[dev], __ATOMIC_ACQUIRE)) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_prefix_partial_mfma_kernel<false>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, PP_LDS);
      if (e != hipSuccess) {
        mh_set_error("attn_prefix_partial: cannot raise dynamic LDS to %d bytes: %s", PP_LDS, hipGetErrorString(e));
        return MH_ERR_LAUNCH;
      }
      __atomic_store_n(&attr_set_of[dev], true, __ATOMIC_RELEASE);
    }
    attn_prefix_partial_mfma_kernel<false><<<H * nch, 256, PP_LDS, st>>>((const bf16*)qkv, cos_t, sin_t, (const bf16*)kpre,
                                                                         (const bf16*)vpre, ws, (int)B, H, (int)Pmax, nch,
                                                                         (int)pre_len, (int)pos, scale, pre_len_dev, pos_dev, nullptr);
  } else {
    attn_prefix_partial_valu_kernel<float><<<dim3(H * nch, (unsigned)B), 256, 0, st>>>(
        (const float*)qkv, cos_t, sin_t, (const float*)kpre, (const float*)vpre, ws, (int)B, H, (int)Pmax, nch, (int)pre_len,
        (int)pos, scale, pre_len_dev, pos_dev);
  }
  MH_LAUNCH_CHECK();
  return MH_OK;
}

// The slots form (the header of this file): G prompts, every row at its own position and in at most one slot.
extern "C" int mh_attn_prefix_partial_slots(const void* qkv, const float* cos_t, const float* sin_t, const void* kpre,
                                            const void* vpre, const int32_t* slot_len, const int32_t* row_slot,
                                            const int32_t* row_pos, float* ws, int64_t ws_floats, int64_t B, int H, int hd,
                                            int64_t G, int64_t Pmax, float scale, int dtype, void* stream) {
  MH_REQUIRE(hd == 64, "attn_prefix_partial_slots: head_dim %d unsupported (64)", hd);
  MH_REQUIRE(dtype == MH_BF16 || dtype == MH_F32, "attn_prefix_partial_slots: bad dtype %d", dtype);
  MH_REQUIRE(qkv != nullptr, "attn_prefix_partial_slots: qkv is NULL");
  MH_REQUIRE(cos_t != nullptr && sin_t != nullptr, "attn_prefix_partial_slots: a rope table is NULL (qkv arrives unrotated)");
  MH_REQUIRE(kpre != nullptr && vpre != nullptr, "attn_prefix_partial_slots: kpre or vpre is NULL");
  MH_REQUIRE(slot_len != nullptr, "attn_prefix_partial_slots: slot_len is NULL (one device int32 length per slot)");
  MH_REQUIRE(row_slot != nullptr, "attn_prefix_partial_slots: row_slot is NULL (one device int32 slot id per row, -1: none)");
  MH_REQUIRE(row_pos != nullptr, "attn_prefix_partial_slots: row_pos is NULL (one device int32 position per row)");
  MH_REQUIRE(ws != nullptr, "attn_prefix_partial_slots: ws is NULL");
  MH_REQUIRE(G >= 1 && G <= 65535, "attn_prefix_partial_slots: %ld slots (1 to 65535)", (long)G);
  MH_REQUIRE(B > 0 && B <= PP_MAX_ROWS && H > 0 && Pmax > 0 && Pmax < (1 << 24),
             "attn_prefix_partial_slots: bad args B=%ld (at most %d: a slot's member list lives in LDS) H=%d Pmax=%ld", (long)B,
             PP_MAX_ROWS, H, (long)Pmax);
  const int nch = (int)((Pmax + PREFIX_CHUNK - 1) / PREFIX_CHUNK);
  MH_REQUIRE(ws_floats >= prefix_ws_floats(B, H, nch), "attn_prefix_partial_slots: workspace of %ld floats, %ld needed",
             (long)ws_floats, (long)prefix_ws_floats(B, H, nch));
  MH_REQUIRE((int64_t)H * nch < (1 << 30), "attn_prefix_partial_slots: grid too large");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MH_BF16) {
    constexpr int MAX_DEV = 64;
    constexpr int LDS_MAX = PP_LDS + 4 * PP_MAX_ROWS;
    static bool attr_set_of[MAX_DEV];
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) {
      mh_set_error("attn_prefix_partial_slots: no current device (or ordinal %d beyond %d)", dev, MAX_DEV - 1);
      return MH_ERR_LAUNCH;
    }
    if (!__atomic_load_n(&attr_set_of[dev], __ATOMIC_ACQUIRE)) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_prefix_partial_mfma_kernel<true>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
      if (e != hipSuccess) {
        mh_set_error("attn_prefix_partial_slots: cannot raise dynamic LDS to %d bytes: %s", LDS_MAX, hipGetErrorString(e));
        return MH_ERR_LAUNCH;
      }
      __atomic_store_n(&attr_set_of[dev], true, __ATOMIC_RELEASE);
    }
    const int lds = PP_LDS + 4 * (int)((B + 63) / 64 * 64);
    attn_prefix_partial_mfma_kernel<true><<<dim3(H * nch, (unsigned)G), 256, lds, st>>>(
        (const bf16*)qkv, cos_t, sin_t, (const bf16*)kpre, (const bf16*)vpre, ws, (int)B, H, (int)Pmax, nch, 0, 0, scale, slot_len,
        row_pos, row_slot);
  } else {
    attn_prefix_partial_valu_kernel<float, true><<<dim3(H * nch, (unsigned)B), 256, 0, st>>>(
        (const float*)qkv, cos_t, sin_t, (const float*)kpre, (const float*)vpre, ws, (int)B, H, (int)Pmax, nch, 0, 0, scale,
        slot_len, row_pos, row_slot, (int)G);
  }
  MH_LAUNCH_CHECK();
  return MH_OK;
}
