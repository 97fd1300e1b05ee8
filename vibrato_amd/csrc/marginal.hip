// Lattice marginals (MeCab's -m / -l 2 with -t): the posterior probability of every node of the lattice the
// 1-best path is taken from, under P(path) ~ exp(-cost / T), one wavefront per sentence, in a translation unit of its own (nothing
// shared with lattice.hip / fused.hip / nbest.hip but device_common.hpp; the phases up to the forward sweep are
// lattice_forward.hpp's, which sample.hip instantiates too).  Where the sweep of Lattice::insert_node (lattice.rs:103-151)
// keeps ONE (min_cost, back pointer) per node, this kernel keeps two float64 per node: alpha, the log of the summed weight of the
// partial paths from BOS that end in the node, and beta, the log of the summed weight of the partial paths from the node to EOS
// (the node's own word cost belongs to alpha).  log Z = alpha(EOS), P(node) = exp(alpha + beta - log Z).
//
// Forward: the step records in order, a candidate owns a row of 16 lanes, the lanes stride its predecessors.  Backward: the step
// records in REVERSE, a predecessor owns the row, the lanes stride the candidates -- the transposed walk over the same staged
// connection costs conn[soff + j * nc + ci].  Every lane keeps a running (maximum, sum of exp(x - maximum)) pair, the 16 pairs of a
// row are combined with four DPP steps on the two halves of the doubles; a step of any size needs no other state.  Costs are exact:
// int16 / int32 cells and int16 word costs go to float64 one by one, nothing is summed in i32, so nothing wraps.
#include "lattice_forward.hpp"

namespace vbt {
namespace {

// What follows the shared forward sweep (lattice_forward.hpp: P0-P4) for the marginals: the backward sweep and the emit.
template <bool kWide>
struct MarginalTail {
    static constexpr bool kBeta = true, kOrderedLists = false;
    const BatchArgs& A;
    const MarginalArgs& M;
    uint32_t sid;
    __device__ __forceinline__ uint64_t aux_bytes(uint32_t, uint32_t, uint64_t E) const { return 8 * E; }
    // an empty sentence (worker.rs:50-52), or one whose every character is a skipped space: no nodes, log Z = 0
    __device__ __forceinline__ void none(bool) const {
        if (threadIdx.x == 0) { A.tok_cnt[sid] = 0; M.log_z[sid] = 0.0; }
    }
    template <typename Ctx, typename Gather, typename StepPairs>
    __device__ __forceinline__ uint64_t run(const Ctx& X, Gather& gather, StepPairs& step_pairs) const {
        typedef typename std::conditional<kWide, int32_t, int16_t>::type ConnT;
        typedef typename std::remove_const<typename std::remove_pointer<decltype(X.c2b)>::type>::type IdxT;
        const uint32_t ln = threadIdx.x;
        const uint64_t lt_mask = (1ull << ln) - 1ull;
        const uint32_t row = ln >> 4, l = ln & (kRowLanes - 1);
        const uint32_t n = X.n, C = X.C, S = X.S, es_eos = X.es_eos;
        const IdxT *c2b = X.c2b, *cand_off = X.cand_off, *nd_end = X.nd_end, *nd_eslot = X.nd_eslot;
        const StepRec<IdxT>* st = X.st;
        double *e_alpha = X.e_alpha, *e_beta = static_cast<double*>(X.aux);  // beta: ... of the paths node -> EOS (-inf: nothing follows it)
        const uint32_t* nd_word = X.nd_word;
        const int16_t* nd_wcost = X.nd_wcost;
        const ConnT* conn = X.conn;
        const uint64_t q_cap = X.q_cap;
        uint32_t st_lo = X.st_lo, st_hi = X.st_hi;
        const double nit = X.nit;
        // ---- P5: backward, the step records in reverse.  beta_j = LSE_c(-(conn(j, c) + w_c) / T + beta_c) for every predecessor slot
        // of the step (an end list is the predecessor list of exactly one step: written once): the PREDECESSOR owns the row, the lanes
        // walk the candidates -- consecutive cells of conn.  Blocks of whole steps from the back; what the staging still holds is not
        // gathered again (all pairs fit: nothing is) ----
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
                for (uint32_t jb = 0; jb < np; jb += kRows) {
                    const uint32_t j = jb + row;
                    const bool live_row = j < np;
                    const ConnT* cells = conn + soff + (size_t)(live_row ? j : 0u) * nc;
                    double m = kNegInf, s = 0.0;
                    if (live_row)
                        for (uint32_t t = l; t < nc; t += kRowLanes) {
                            const uint32_t c = c_beg + t;
                            const double b = e_beta[nd_eslot[c]];
                            if (b != kNegInf) lse_add(m, s, b + ((double)cells[t] + (double)nd_wcost[c]) * nit);
                        }
                    row_lse(m, s);
                    if (live_row && l == 0) e_beta[p_beg + j] = s > 0.0 ? m + log(s) : kNegInf;
                }
                __syncthreads();
            }
            kend = k;
        }

        // ---- P6: emit.  prob_c = exp(alpha_c + beta_c - log Z), kept where alpha was; the nodes that pass are counted with ballot /
        // popcount, the sentence takes its range of the staging with ONE atomic add, the records go there in lattice order ----
        const double log_z = e_alpha[es_eos];
        uint32_t count = 0;
        for (uint32_t c0 = 0; c0 < C; c0 += 64) {
            const uint32_t c = c0 + ln;
            bool pass = false;
            if (c < C) {
                const uint32_t es = nd_eslot[c];
                double p = exp(e_alpha[es] + e_beta[es] - log_z);  // (-inf on either side: 0; log Z = -inf, no path at all: NaN, dropped)
                p = p > 1.0 ? 1.0 : p;
                pass = p > 0.0 && p >= M.min_prob;
                e_alpha[es] = pass ? p : 0.0;
            }
            count += (uint32_t)__popcll(__ballot(pass));
        }
        __syncthreads();
        unsigned long long base = 0;
        if (M.rerun) base = M.node_base[sid];  // the range this sentence took when it found the staging full
        else if (ln == 0) base = atomicAdd(M.stage_cursor, (unsigned long long)count);
        base = uniform64(base);
        if (ln == 0) {
            A.tok_cnt[sid] = count;
            M.log_z[sid] = log_z;
            M.node_base[sid] = base;
        }
        if (base + count > M.stage_cap) {  // full: the host makes room for the cursor's final value and runs this sentence again
            if (ln == 0) {
                if (M.rerun) atomicOr(&A.ctrl[kError], (uint32_t)kErrTokCap);
                else M.oflow_list[atomicAdd(M.oflow_count, 1u)] = sid;
            }
            return 0;
        }
        vbt_marginal_node* outp = M.stage + base;
        uint32_t done = 0;
        for (uint32_t c0 = 0; c0 < C; c0 += 64) {
            const uint32_t c = c0 + ln;
            double p = 0.0;
            if (c < C) p = e_alpha[nd_eslot[c]];
            const uint64_t mk = __ballot(p > 0.0);
            if (p > 0.0) {
                uint32_t lo = 0, hi = n;  // start position = the one whose candidate range contains c
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if ((uint32_t)cand_off[mid + 1] <= c) lo = mid + 1; else hi = mid;
                }
                const uint32_t en = nd_end[c];
                vbt_marginal_node r;
                r.start_char = lo; r.end_char = en;
                r.start_byte = c2b[lo]; r.end_byte = c2b[en];
                r.word_idx = nd_word[c];
                r.reserved = 0;
                r.prob = p;
                outp[done + (uint32_t)__popcll(mk & lt_mask)] = r;
            }
            done += (uint32_t)__popcll(mk);
        }
        return 0;
    }
};

template <typename IdxT, bool kGlobal, bool kWide>
__device__ __forceinline__ uint64_t marginal_sentence(const DevDict& D, const BatchArgs& A, const MarginalArgs& M, uint32_t sid, char* abase, uint64_t acap) {
    return forward_sentence<IdxT, kGlobal, kWide>(D, A, M.neg_inv_t, M.stage_cells, sid, abase, acap, MarginalTail<kWide>{A, M, sid});
}

// LDS tier: one wavefront per sentence (block b = sentence b), the arena in `lds_bytes` of dynamic LDS; what does not fit is
// filed for the slab tier.
template <bool kWide>
__global__ void __launch_bounds__(64) marginal_lds(DevDict D, BatchArgs A, MarginalArgs M, uint32_t lds_bytes, uint32_t* out_list, uint32_t* out_count) {
    if (batch_rejected(A)) return;
    const uint32_t sid = blockIdx.x;
    if (marginal_sentence<uint16_t, false, kWide>(D, A, M, sid, g_smem, lds_bytes) != 0 && threadIdx.x == 0) out_list[atomicAdd(out_count, 1u)] = sid;
}

// Slab tier: persistent waves, the arena in a private slab of global memory taken from the scratch bump allocator (any length).
template <bool kWide>
__global__ void __launch_bounds__(64) marginal_slab(DevDict D, BatchArgs A, MarginalArgs M, const uint32_t* in_list, const uint32_t* in_count, uint32_t* cursor) {
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
            const uint64_t need = marginal_sentence<uint32_t, true, kWide>(D, A, M, sid, slab, slab_bytes);
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
                    M.log_z[sid] = 0.0;
                }
                break;
            }
            __syncthreads();
        }
        __syncthreads();
    }
}

// ---- pack pass: node_off[n + 1] and the records in sentence order.  Tiles of 256 sentences.
constexpr uint32_t kPackTile = 256;
__global__ void __launch_bounds__(256) marginal_tile_sums(BatchArgs A, MarginalArgs M) {
    __shared__ uint32_t ws[4];
    const uint64_t i = (uint64_t)blockIdx.x * kPackTile + threadIdx.x;
    uint32_t tot;
    block_exscan(i < A.n ? A.tok_cnt[i] : 0u, ws, tot);
    if (threadIdx.x == 0) M.tile_nodes[blockIdx.x] = tot;
}
// one workgroup: exclusive prefix of the tiles' sums in place; totals[0] = nodes = node_off[n]
__global__ void __launch_bounds__(256) marginal_tile_scan(BatchArgs A, MarginalArgs M, uint32_t n_tiles) {
    __shared__ uint32_t ws[4];
    uint32_t run = 0;
    if (!batch_rejected(A))
        for (uint32_t t0 = 0; t0 < n_tiles; t0 += 256) {
            const uint32_t t = t0 + threadIdx.x;
            uint32_t tot;
            const uint32_t ex = block_exscan(t < n_tiles ? M.tile_nodes[t] : 0u, ws, tot);
            if (t < n_tiles) M.tile_nodes[t] = run + ex;
            run += tot;
        }
    if (threadIdx.x == 0) { M.totals[0] = run; M.node_off[A.n] = run; }
}
__global__ void __launch_bounds__(256) marginal_pack(BatchArgs A, MarginalArgs M) {
    __shared__ uint32_t ws[4];
    __shared__ uint64_t src[kPackTile];
    __shared__ uint32_t dst[kPackTile], num[kPackTile];
    if (batch_rejected(A)) return;
    const uint64_t i = (uint64_t)blockIdx.x * kPackTile + threadIdx.x;
    const uint32_t cnt = i < A.n ? A.tok_cnt[i] : 0u;
    uint32_t tot;
    const uint32_t q = M.tile_nodes[blockIdx.x] + block_exscan(cnt, ws, tot);
    num[threadIdx.x] = cnt;
    dst[threadIdx.x] = q;
    src[threadIdx.x] = cnt ? M.node_base[i] : 0ull;
    if (i < A.n) M.node_off[i] = q;
    __syncthreads();
    // a wave per sentence, 16 bytes per lane: a record is two of them
    for (uint32_t rw = threadIdx.x >> 6; rw < kPackTile; rw += 4) {
        const uint32_t quads = num[rw] * 2u;
        if (!quads) continue;
        const uint4* __restrict__ from = reinterpret_cast<const uint4*>(M.stage + src[rw]);
        uint4* __restrict__ to = reinterpret_cast<uint4*>(M.nodes + dst[rw]);
        for (uint32_t w = threadIdx.x & 63u; w < quads; w += 64) to[w] = from[w];
    }
}

}  // namespace

namespace kern {

void marginal_lds(uint32_t n, uint32_t lds_bytes, hipStream_t stream, const DevDict& D, const BatchArgs& a, const MarginalArgs& m, uint32_t* out_list, uint32_t* out_count) {
    hipLaunchKernelGGL(D.matrix_wide ? vbt::marginal_lds<true> : vbt::marginal_lds<false>, dim3(n), dim3(64), lds_bytes, stream, D, a, m, lds_bytes, out_list, out_count);
}
void marginal_slab(uint32_t workgroups, hipStream_t stream, const DevDict& D, const BatchArgs& a, const MarginalArgs& m, const uint32_t* in_list, const uint32_t* in_count, uint32_t* cursor) {
    hipLaunchKernelGGL(D.matrix_wide ? vbt::marginal_slab<true> : vbt::marginal_slab<false>, dim3(workgroups), dim3(64), 0, stream, D, a, m, in_list, in_count, cursor);
}
void marginal_pack(hipStream_t stream, const BatchArgs& a, const MarginalArgs& m) {
    const uint32_t n_tiles = (a.n + kPackTile - 1) / kPackTile;
    hipLaunchKernelGGL(vbt::marginal_tile_sums, dim3(n_tiles), dim3(256), 0, stream, a, m);
    hipLaunchKernelGGL(vbt::marginal_tile_scan, dim3(1), dim3(256), 0, stream, a, m, n_tiles);
    hipLaunchKernelGGL(vbt::marginal_pack, dim3(n_tiles), dim3(256), 0, stream, a, m);
}

}  // namespace kern
}  // namespace vbt
