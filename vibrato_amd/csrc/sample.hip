// Sampled segmentations: whole paths drawn from P(path) ~ exp(-cost / T) over the lattice the 1-best path is
// taken from -- forward filtering / backward sampling, one wavefront per sentence.  The forward half is lattice_forward.hpp's (P0-P4,
// shared with marginal.hip): it leaves alpha for every end-list slot.  This file adds the backward half: the samples of a sentence
// walk from EOS to BOS over the step records in REVERSE, in lockstep with the blocks of steps the connection-cost staging holds
// (what the marginals' backward sweep does with the same blocks), and the emit.  No beta, no per-node records, no overflow
// protocol: a sentence of n characters yields at most n_samples x n token records.
//
// At a step, the samples whose current node is a candidate of the step are active (a ballot).  An active sample owns a DPP row of
// 16 lanes, four samples per wave pass.  With c the current node, its predecessors j (the step's end list, in end-list order) weigh
// p_j = exp(alpha_j - conn(j, c) / T - L_c), L_c = alpha_c + w_c / T = the log of their sum, known from the forward sweep: no
// maximum pass.  Lane l sums the p_j of the l-th contiguous chunk of ceil(np / 16) predecessors, a DPP row scan (row_shr 1, 2, 4, 8)
// gives the inclusive prefixes, the last lane's is the total.  With thr = u x total, the first lane of positive chunk sum whose
// inclusive prefix exceeds thr walks its chunk once more, from the exclusive prefix, and takes the first j whose running sum
// exceeds thr (rounding left none: its last j of positive weight; no such lane: the last lane of positive sum, its last j of
// positive weight).  The node in end-list slot p_beg + j is the sample's next current node; slot 0 is BOS and ends the walk.
//
// u = (x + 0.5) / 2^32, x = word 0 of Philox4x32-10 at counter (lo32(s), hi32(s), r, t), key (lo32(seed), hi32(seed)): s the
// sentence's index in the whole call, r the sample, t the draw (0 at EOS, + 1 per token).  End lists are in the reference's insertion
// order (lattice_forward.hpp: kOrderedLists), so a result depends on the text, the dictionary, T, n_samples, seed and s only.
#include "lattice_forward.hpp"

namespace vbt {
namespace {

// word 0 of Philox4x32-10 (Salmon et al., SC'11): ten rounds of two 32 x 32 -> 64 multiplications, the key bumped between rounds
__device__ __forceinline__ uint32_t philox4x32_10_w0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0;
        c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

// inclusive prefix sums over the 16 lanes of a DPP row, in every lane its own: row_shr 1, 2, 4, 8 (a lane without a source adds 0).
// No LDS traffic.  Every lane of the wave must be active.
__device__ __forceinline__ double row_scan(double x) {
    x += dpp_f64<0x111>(x);
    x += dpp_f64<0x112>(x);
    x += dpp_f64<0x114>(x);
    x += dpp_f64<0x118>(x);
    return x;
}

constexpr uint32_t kWalkDone = 0xFFFFFFFFu;  // current node of a sample that has reached BOS

// What follows the shared forward sweep for the samples.  The aux region holds the walk state: per sample its current node and
// its token count (the draw number), then its token list in reverse order, at most n + 1 entries of IdxT.
template <typename IdxT, bool kWide>
struct SampleTail {
    static constexpr bool kBeta = false, kOrderedLists = true;
    const BatchArgs& A;
    const SampleArgs& P;
    uint32_t sid;
    __device__ __forceinline__ uint64_t aux_bytes(uint32_t n, uint32_t C, uint64_t) const {
        const uint64_t walk = (uint64_t)P.k * (8 + ((uint64_t)n + 1) * sizeof(IdxT));
        return walk > 2ull * C ? walk : 2ull * C;
    }
    // an empty sentence: no paths; every character a skipped space: n_samples paths of no tokens; log Z = 0 either way
    __device__ __forceinline__ void none(bool spaces_only) const {
        const uint32_t ln = threadIdx.x;
        if (ln == 0) { A.tok_cnt[sid] = spaces_only ? P.k : 0u; P.log_z[sid] = 0.0; }
        if (ln < P.k) {
            const size_t i = (size_t)sid * P.k + ln;
            P.path_cnt[i] = 0; P.path_cost[i] = 0; P.path_base[i] = 0;
        }
    }
    template <typename Ctx, typename Gather, typename StepPairs>
    __device__ __forceinline__ uint64_t run(const Ctx& X, Gather& gather, StepPairs& step_pairs) const {
        typedef typename std::conditional<kWide, int32_t, int16_t>::type ConnT;
        const uint32_t ln = threadIdx.x;
        const uint32_t row = ln >> 4, l = ln & (kRowLanes - 1);
        const uint32_t n = X.n, C = X.C, S = X.S, K = P.k;
        const IdxT *c2b = X.c2b, *cand_off = X.cand_off, *nd_end = X.nd_end, *nd_eslot = X.nd_eslot, *e_node = X.e_node;
        const StepRec<IdxT>* st = X.st;
        const double* e_alpha = X.e_alpha;
        const int16_t* nd_wcost = X.nd_wcost;
        const ConnT* conn = X.conn;
        const uint64_t q_cap = X.q_cap;
        uint32_t st_lo = X.st_lo, st_hi = X.st_hi;
        const double nit = X.nit;
        uint32_t* cur = static_cast<uint32_t*>(X.aux);
        uint32_t* cnt = cur + K;
        IdxT* toks = reinterpret_cast<IdxT*>(cnt + K);
        const size_t tstride = (size_t)n + 1;

        const double log_z = e_alpha[X.es_eos];
        if (!(log_z > kNegInf)) {  // no path reaches EOS: nothing to draw from
            if (ln == 0) { A.tok_cnt[sid] = 0; P.log_z[sid] = log_z; }
            return 0;
        }
        __syncthreads();  // (the forward sweep's last reads of the aux region's neighbours are done)
        if (ln < K) { cur[ln] = C; cnt[ln] = 0; }  // every sample starts at EOS (node C)
        const uint64_t s_glob = P.sid_base + sid;
        const uint32_t s_lo = (uint32_t)s_glob, s_hi = (uint32_t)(s_glob >> 32), k_lo = (uint32_t)P.seed, k_hi = (uint32_t)(P.seed >> 32);

        // ---- P5: the walks, the step records in reverse; blocks of whole steps from the back as the marginals' backward sweep
        // takes them: what the staging still holds is not gathered again ----
        for (uint32_t kend = S; kend > 0;) {
            uint32_t k = kend;
            uint64_t q = 0;
            while (k > 0) {
                const uint64_t pairs = step_pairs(k - 1);
                if (q + pairs > q_cap) break;
                q += pairs;
                --k;
            }
            if (k != st_lo || kend != st_hi) {
                __syncthreads();
                gather(k, kend);
                st_lo = k; st_hi = kend;
            }
            __syncthreads();
            uint32_t soff = (uint32_t)q;
            for (uint32_t kk = kend; kk-- > k;) {
                const StepRec<IdxT> sr = st[kk];
                const uint32_t c_beg = __builtin_amdgcn_readfirstlane((uint32_t)sr.cbeg);
                const uint32_t nc = __builtin_amdgcn_readfirstlane((uint32_t)sr.nc);
                const uint32_t p_beg = __builtin_amdgcn_readfirstlane((uint32_t)sr.pbeg);
                const uint32_t np = __builtin_amdgcn_readfirstlane((uint32_t)sr.np);
                soff -= nc * np;
                const uint32_t mine = ln < K ? cur[ln] : kWalkDone;
                uint64_t act = __ballot(mine - c_beg < nc);  // the samples whose current node is a candidate of this step
                if (!act) continue;
                const uint32_t chunk = (np + kRowLanes - 1) / kRowLanes;
                const uint32_t j0 = l * chunk < np ? l * chunk : np, j1 = j0 + chunk < np ? j0 + chunk : np;
                while (act) {
                    uint32_t r = 64;  // row i takes the i-th lowest active sample
                    for (uint32_t i = 0; i < kRows; ++i)
                        if (act) {
                            if (i == row) r = (uint32_t)__builtin_ctzll(act);
                            act &= act - 1;
                        }
                    const bool live = r < 64;
                    const uint32_t c = live ? cur[r] : c_beg;
                    const uint32_t t = live ? cnt[r] : 0u;
                    const double L_c = e_alpha[nd_eslot[c]] - (double)nd_wcost[c] * nit;  // alpha_c + w_c / T
                    const ConnT* col = conn + soff + (c - c_beg);
                    auto weight = [&](uint32_t j) -> double {
                        const double a = e_alpha[p_beg + j];
                        return a == kNegInf ? 0.0 : exp(a + (double)col[(size_t)j * nc] * nit - L_c);
                    };
                    double s = 0.0;
                    if (live)
                        for (uint32_t j = j0; j < j1; ++j) s += weight(j);
                    const double incl = row_scan(s);
                    const double excl = dpp_f64<0x111>(incl);
                    const double total = __shfl(incl, (int)(row * kRowLanes + kRowLanes - 1));
                    const double u = ((double)philox4x32_10_w0(s_lo, s_hi, r, t, k_lo, k_hi) + 0.5) * (1.0 / 4294967296.0);
                    const double thr = u * total;
                    const uint32_t over = (uint32_t)(__ballot(live && s > 0.0 && incl > thr) >> (row * kRowLanes)) & 0xFFFFu;
                    const uint32_t some = (uint32_t)(__ballot(live && s > 0.0) >> (row * kRowLanes)) & 0xFFFFu;
                    const uint32_t lsel = over ? (uint32_t)__builtin_ctz(over) : some ? 31u - (uint32_t)__builtin_clz(some) : kRowLanes;
                    if (live && l == lsel) {
                        uint32_t jsel = kWalkDone, jlast = kWalkDone;
                        double run = excl;
                        for (uint32_t j = j0; j < j1 && jsel == kWalkDone; ++j) {
                            const double p = weight(j);
                            if (p > 0.0) {
                                jlast = j;
                                run += p;
                                if (over && run > thr) jsel = j;
                            }
                        }
                        if (jsel == kWalkDone) jsel = jlast;
                        if (jsel != kWalkDone) {  // (s > 0: the chunk has a positive weight)
                            const uint32_t nx = e_node[p_beg + jsel];
                            if (nx == C + 1 || t >= tstride) cur[r] = kWalkDone;  // BOS (tokens <= characters: the bound keeps a corrupted walk finite)
                            else {
                                cur[r] = nx;
                                toks[(size_t)r * tstride + t] = (IdxT)nx;
                                cnt[r] = t + 1;
                            }
                        }
                    }
                }
                __syncthreads();
            }
            kend = k;
        }

        // ---- P6: emit.  The sentence takes its range of the staging with ONE atomic add, sample r the tokens behind those of the
        // samples below it; a wave writes a path's records in sentence order, 64 tokens at a time: the cost of a token's step
        // (connection + word) straight from the matrix, its running sum by a wave scan in int64 (total_cost = its low 32 bits) ----
        const uint32_t T = ln < K ? cnt[ln] : 0u;
        uint32_t tot;
        const uint32_t ex = wave_exscan(T, tot);
        unsigned long long base = 0;
        if (ln == 0) base = atomicAdd(P.stage_cursor, (unsigned long long)tot);
        base = uniform64(base);
        if (base + tot > P.stage_cap) {  // cannot happen within the workspace's bound (tokens <= bytes per sample); nothing is written
            if (ln == 0) { atomicOr(&A.ctrl[kError], (uint32_t)kErrTokCap); A.tok_cnt[sid] = 0; P.log_z[sid] = log_z; }
            return 0;
        }
        if (ln == 0) { A.tok_cnt[sid] = K; P.log_z[sid] = log_z; }
        if (ln < K) {
            P.path_cnt[(size_t)sid * K + ln] = T;
            P.path_base[(size_t)sid * K + ln] = base + ex;
        }
        const ConnT* __restrict__ matrix = X.matrix;
        const uint32_t NR = X.NR;
        for (uint32_t r = 0; r < K; ++r) {
            const uint32_t Tr = (uint32_t)__shfl((int)T, (int)r);
            vbt_token_rec* outp = P.stage + base + (uint32_t)__shfl((int)ex, (int)r);
            const IdxT* tk = toks + (size_t)r * tstride;  // reverse order: tk[Tr - 1] is the first token
            long long carry = 0;
            for (uint32_t i0 = 0; i0 < Tr; i0 += 64) {
                const uint32_t i = i0 + ln;
                const bool valid = i < Tr;
                uint32_t c = 0;
                long long x = 0;
                if (valid) {
                    c = tk[Tr - 1 - i];
                    const uint32_t right = i ? X.e_right[nd_eslot[tk[Tr - i]]] : 0u;  // BOS: right id 0
                    x = (long long)matrix[(size_t)X.nd_left[c] * NR + right] + (long long)nd_wcost[c];
                }
                for (uint32_t o = 1; o < 64; o <<= 1) {
                    const long long y = __shfl_up(x, o);
                    if (ln >= o) x += y;
                }
                x += carry;
                if (valid) {
                    uint32_t lo = 0, hi = n;  // start position = the one whose candidate range contains c
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if ((uint32_t)cand_off[mid + 1] <= c) lo = mid + 1; else hi = mid;
                    }
                    const uint32_t en = nd_end[c];
                    vbt_token_rec rec;
                    rec.start_char = lo; rec.end_char = en;
                    rec.start_byte = c2b[lo]; rec.end_byte = c2b[en];
                    rec.word_idx = X.nd_word[c];
                    rec.total_cost = (int32_t)(uint32_t)(unsigned long long)x;  // accumulated along THIS path, wrapping as i32 does
                    outp[i] = rec;
                }
                carry = __shfl(x, 63);
            }
            if (ln == 0) {  // + the connection into EOS (left id of node C)
                const uint32_t right = Tr ? X.e_right[nd_eslot[tk[0]]] : 0u;
                P.path_cost[(size_t)sid * K + r] = carry + (long long)matrix[(size_t)X.nd_left[C] * NR + right];
            }
        }
        return 0;
    }
};

template <typename IdxT, bool kGlobal, bool kWide>
__device__ __forceinline__ uint64_t sample_sentence(const DevDict& D, const BatchArgs& A, const SampleArgs& P, uint32_t sid, char* abase, uint64_t acap) {
    return forward_sentence<IdxT, kGlobal, kWide>(D, A, P.neg_inv_t, P.stage_cells, sid, abase, acap, SampleTail<IdxT, kWide>{A, P, sid});
}

// LDS tier: one wavefront per sentence (block b = sentence b), the arena in `lds_bytes` of dynamic LDS; what does not fit is
// filed for the slab tier.
template <bool kWide>
__global__ void __launch_bounds__(64) sample_lds(DevDict D, BatchArgs A, SampleArgs P, uint32_t lds_bytes, uint32_t* out_list, uint32_t* out_count) {
    if (batch_rejected(A)) return;
    const uint32_t sid = blockIdx.x;
    if (sample_sentence<uint16_t, false, kWide>(D, A, P, sid, g_smem, lds_bytes) != 0 && threadIdx.x == 0) out_list[atomicAdd(out_count, 1u)] = sid;
}

// Slab tier: persistent waves, the arena in a private slab of global memory taken from the scratch bump allocator (any length).
template <bool kWide>
__global__ void __launch_bounds__(64) sample_slab(DevDict D, BatchArgs A, SampleArgs P, const uint32_t* in_list, const uint32_t* in_count, uint32_t* cursor) {
    if (batch_rejected(A)) return;
    const uint32_t count = *in_count;
    char* slab = nullptr;
    uint64_t slab_bytes = 0;
    unsigned long long* bump = reinterpret_cast<unsigned long long*>(&A.ctrl[kBump]);
    for (bool first = true;; first = false) {
        uint32_t k = blockIdx.x;
        if (!first) {
            if (threadIdx.x == 0) k = gridDim.x + atomicAdd(cursor, 1u);
            k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
        }
        if (k >= count) break;
        const uint32_t sid = in_list[k];
        for (int attempt = 0; attempt < 6; ++attempt) {
            const uint64_t need = sample_sentence<uint32_t, true, kWide>(D, A, P, sid, slab, slab_bytes);
            if (need == 0) break;
            bool failed = need == kNoFit || attempt == 5;
            if (!failed) {  // grow: a fresh slab from the bump arena
                uint64_t want = need + need / 4 + 4096;
                want = (want + 255) & ~255ull;
                unsigned long long off = 0;
                if (threadIdx.x == 0) off = atomicAdd(bump, (unsigned long long)want);
                off = uniform64(off);
                if (off + want > A.scratch_bytes) failed = true;
                else { slab = A.scratch + off; slab_bytes = want; }
            }
            if (failed) {
                if (threadIdx.x == 0) {
                    atomicOr(&A.ctrl[kError], need == kNoFit ? (uint32_t)kErrTooLong : (uint32_t)kErrScratch);
                    A.tok_cnt[sid] = 0;
                    P.log_z[sid] = 0.0;
                }
                break;
            }
            __syncthreads();
        }
        __syncthreads();
    }
}

// ---- pack pass: (sentence, sample) is a row; row i = s * k + r exists when r < tok_cnt[s] (k or 0).  Tiles of 256 rows, laid out
// as nbest's; the cost of a path is int64 here and a row's records sit at path_base[i] of the staging.
constexpr uint32_t kPackTile = 256;
__device__ __forceinline__ void pack_row(const BatchArgs& A, const SampleArgs& P, uint64_t i, uint32_t& exists, uint32_t& cnt) {
    exists = 0; cnt = 0;
    if (i < (uint64_t)A.n * P.k) {
        const uint32_t s = (uint32_t)(i / P.k), r = (uint32_t)(i - (uint64_t)s * P.k);
        exists = r < A.tok_cnt[s] ? 1u : 0u;
        cnt = exists ? P.path_cnt[i] : 0u;
    }
}
__global__ void __launch_bounds__(256) sample_tile_sums(BatchArgs A, SampleArgs P) {
    __shared__ uint32_t ws[4];
    uint32_t exists, cnt, tp, tt;
    pack_row(A, P, (uint64_t)blockIdx.x * kPackTile + threadIdx.x, exists, cnt);
    block_exscan(exists, ws, tp);
    block_exscan(cnt, ws, tt);
    if (threadIdx.x == 0) { P.tile_paths[blockIdx.x] = tp; P.tile_toks[blockIdx.x] = tt; }
}
// one workgroup: exclusive prefix of the tiles' sums in place; totals[0] = paths, totals[1] = tokens, path_off[n], tok_off[paths]
__global__ void __launch_bounds__(256) sample_tile_scan(BatchArgs A, SampleArgs P, uint32_t n_tiles) {
    __shared__ uint32_t ws[4];
    uint32_t run_p = 0, run_t = 0;
    if (!batch_rejected(A))
        for (uint32_t t0 = 0; t0 < n_tiles; t0 += 256) {
            const uint32_t t = t0 + threadIdx.x;
            const uint32_t vp = t < n_tiles ? P.tile_paths[t] : 0u, vt = t < n_tiles ? P.tile_toks[t] : 0u;
            uint32_t tp, tt;
            const uint32_t ep = block_exscan(vp, ws, tp), et = block_exscan(vt, ws, tt);
            if (t < n_tiles) { P.tile_paths[t] = run_p + ep; P.tile_toks[t] = run_t + et; }
            run_p += tp; run_t += tt;
        }
    if (threadIdx.x == 0) {
        P.totals[0] = run_p; P.totals[1] = run_t;
        P.path_off[A.n] = run_p;
        P.tok_off[run_p] = run_t;
    }
}
// path_off[s], tok_off[p], path_cost[p] and the records, sentence-major, sample-minor
__global__ void __launch_bounds__(256) sample_pack(BatchArgs A, SampleArgs P) {
    __shared__ uint32_t ws[4];
    __shared__ uint64_t src[kPackTile];
    __shared__ uint32_t dst[kPackTile], num[kPackTile];
    if (batch_rejected(A)) return;
    const uint64_t i = (uint64_t)blockIdx.x * kPackTile + threadIdx.x;
    uint32_t exists, cnt, tot;
    pack_row(A, P, i, exists, cnt);
    const uint32_t p = P.tile_paths[blockIdx.x] + block_exscan(exists, ws, tot);
    const uint32_t q = P.tile_toks[blockIdx.x] + block_exscan(cnt, ws, tot);
    num[threadIdx.x] = cnt;
    src[threadIdx.x] = 0;
    dst[threadIdx.x] = 0;
    if (i < (uint64_t)A.n * P.k) {
        const uint32_t s = (uint32_t)(i / P.k), r = (uint32_t)(i - (uint64_t)s * P.k);
        if (r == 0) P.path_off[s] = p;
        if (exists) {
            P.tok_off[p] = q;
            P.path_cost_out[p] = P.path_cost[i];
            src[threadIdx.x] = P.path_base[i];
            dst[threadIdx.x] = q;
        }
    }
    __syncthreads();
    // a wave per row, a dword per lane: records are 6 dwords
    for (uint32_t rw = threadIdx.x >> 6; rw < kPackTile; rw += 4) {
        const uint32_t words = num[rw] * 6u;
        if (!words) continue;
        const uint32_t* __restrict__ from = reinterpret_cast<const uint32_t*>(P.stage + src[rw]);
        uint32_t* __restrict__ to = reinterpret_cast<uint32_t*>(P.tokens + dst[rw]);
        for (uint32_t w = threadIdx.x & 63u; w < words; w += 64) to[w] = from[w];
    }
}

}  // namespace

namespace kern {

void sample_lds(uint32_t n, uint32_t lds_bytes, hipStream_t stream, const DevDict& D, const BatchArgs& a, const SampleArgs& p, uint32_t* out_list, uint32_t* out_count) {
    hipLaunchKernelGGL(D.matrix_wide ? vbt::sample_lds<true> : vbt::sample_lds<false>, dim3(n), dim3(64), lds_bytes, stream, D, a, p, lds_bytes, out_list, out_count);
}
void sample_slab(uint32_t workgroups, hipStream_t stream, const DevDict& D, const BatchArgs& a, const SampleArgs& p, const uint32_t* in_list, const uint32_t* in_count, uint32_t* cursor) {
    hipLaunchKernelGGL(D.matrix_wide ? vbt::sample_slab<true> : vbt::sample_slab<false>, dim3(workgroups), dim3(64), 0, stream, D, a, p, in_list, in_count, cursor);
}
void sample_pack(hipStream_t stream, const BatchArgs& a, const SampleArgs& p) {
    const uint32_t n_tiles = (uint32_t)(((uint64_t)a.n * p.k + kPackTile - 1) / kPackTile);
    hipLaunchKernelGGL(vbt::sample_tile_sums, dim3(n_tiles), dim3(256), 0, stream, a, p);
    hipLaunchKernelGGL(vbt::sample_tile_scan, dim3(1), dim3(256), 0, stream, a, p, n_tiles);
    hipLaunchKernelGGL(vbt::sample_pack, dim3(n_tiles), dim3(256), 0, stream, a, p);
}

}  // namespace kern
}  // namespace vbt
