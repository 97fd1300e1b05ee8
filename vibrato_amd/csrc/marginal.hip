// Lattice marginals (MeCab's -m / -l 2 with -t): the posterior probability of every node of the lattice the
// 1-best path is taken from, under P(path) ~ exp(-cost / T), one wavefront per sentence, in a translation unit of its own (nothing
// shared with lattice.hip / fused.hip / nbest.hip but device_common.hpp).  Where the sweep of Lattice::insert_node (lattice.rs:103-151)
// keeps ONE (min_cost, back pointer) per node, this kernel keeps two float64 per node: alpha, the log of the summed weight of the
// partial paths from BOS that end in the node, and beta, the log of the summed weight of the partial paths from the node to EOS
// (the node's own word cost belongs to alpha).  log Z = alpha(EOS), P(node) = exp(alpha + beta - log Z).
//
// Forward: the step records in order, a candidate owns a row of 16 lanes, the lanes stride its predecessors.  Backward: the step
// records in REVERSE, a predecessor owns the row, the lanes stride the candidates -- the transposed walk over the same staged
// connection costs conn[soff + j * nc + ci].  Every lane keeps a running (maximum, sum of exp(x - maximum)) pair, the 16 pairs of a
// row are combined with four DPP steps on the two halves of the doubles; a step of any size needs no other state.  Costs are exact:
// int16 / int32 cells and int16 word costs go to float64 one by one, nothing is summed in i32, so nothing wraps.
#include "device_common.hpp"

namespace vbt {
namespace {

constexpr double kNegInf = -__builtin_inf();
constexpr uint32_t kRowLanes = 16, kRows = 4;

// one more term x for a running log-sum-exp pair: one exp per term
__device__ __forceinline__ void lse_add(double& m, double& s, double x) {
    if (x == kNegInf) return;
    const double e = exp(-fabs(x - m));  // m == -inf (nothing yet): e = 0 and the pair becomes (x, 1)
    if (x > m) { s = s * e + 1.0; m = x; }
    else s += e;
}
template <int kCtrl>
__device__ __forceinline__ double dpp_f64(double x) {
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, kCtrl, 0xF, 0xF, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), kCtrl, 0xF, 0xF, true);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
template <int kCtrl>
__device__ __forceinline__ void dpp_lse(double& m, double& s) {
    const double m2 = dpp_f64<kCtrl>(m), s2 = dpp_f64<kCtrl>(s);
    const bool mine = m >= m2;
    const double big = mine ? m : m2;
    const double e = exp(-fabs(m - m2));  // (NaN when both are -inf: both sums are 0 then, and the select below drops it)
    const double t = mine ? s + s2 * e : s * e + s2;  // the two lanes of a pair add the same two products: the same bits in both
    s = big == kNegInf ? 0.0 : t;
    m = big;
}
// The pairs of the 16 lanes of a DPP row combined, left in every lane of the row: the two quad permutes, row_half_mirror, row_mirror
// (every lane's pair enters exactly once).  No LDS traffic.  Every lane of the wave must be active.
__device__ __forceinline__ void row_lse(double& m, double& s) {
    dpp_lse<0xB1>(m, s);
    dpp_lse<0x4E>(m, s);
    dpp_lse<0x141>(m, s);
    dpp_lse<0x140>(m, s);
}

// The marginals of sentence `sid` inside the arena [abase, abase + acap).  Returns 0 when done, otherwise the arena bytes it would
// need (kNoFit: never in this tier).  Phases P0-P3a are those of fused.hip's process_sentence (decode, character classes, trie
// walks, unknown words, candidates in reference insertion order, end lists, step records) with this kernel's node layout.
template <typename IdxT, bool kGlobal, bool kWide>
__device__ __forceinline__ uint64_t marginal_sentence(const DevDict& D, const BatchArgs& A, const MarginalArgs& M, uint32_t sid, char* abase, uint64_t acap) {
    typedef typename std::conditional<kWide, int32_t, int16_t>::type ConnT;
    const uint32_t ln = threadIdx.x;
    const uint64_t lt_mask = (1ull << ln) - 1ull;
    constexpr uint64_t kIdxMax = sizeof(IdxT) == 2 ? 0xFFFFull : 0xFFFFFFF0ull;
    const uint64_t b0 = A.offsets[sid], nb64 = A.offsets[sid + 1] - b0;
    auto nothing = [&]() {  // an empty sentence (worker.rs:50-52), or one whose every character is a skipped space: no nodes, log Z = 0
        if (ln == 0) { A.tok_cnt[sid] = 0; M.log_z[sid] = 0.0; }
    };
    if (nb64 == 0) { nothing(); return 0; }
    if (nb64 >= (sizeof(IdxT) == 2 ? 0xFFFFull : 0xFFFFFFFFull)) return kNoFit;
    const uint32_t nb = (uint32_t)nb64;
    const uint8_t* __restrict__ txt = A.text + b0;
    const uint32_t n = count_chars(txt, nb);
    if (n == 0) { nothing(); return 0; }

    Arena ar{abase, acap, 0, true};
    uint32_t* ci = ar.take<uint32_t>(n);            // CharInfo per char
    uint32_t* end_off = ar.take<uint32_t>(n + 2);   // end-list offsets
    uint16_t* code = ar.take<uint16_t>(n);          // system-trie code per char
    uint16_t* ucode = D.has_user ? ar.take<uint16_t>(n) : code;
    IdxT* c2b = ar.take<IdxT>(n + 1);               // char -> byte offset
    IdxT* grp = ar.take<IdxT>(n);                   // groupable run length
    IdxT* cand_off = ar.take<IdxT>(n + 1);          // candidates by start position (CSR)
    uint8_t* reach = ar.take<uint8_t>(n + 1);       // has_previous_node
    if (!ar.ok) return ar.used + (uint64_t)n * 32;  // lower bound; the exact size follows after counting

    // ---- P0: decode, CharInfo, trie codes (Sentence::compute_basic / compute_categories) ----
    {
        uint32_t cb = 0;
        for (uint32_t c0 = 0; c0 < nb; c0 += 64) {
            const uint32_t bi = c0 + ln;
            const uint32_t b = bi < nb ? txt[bi] : 0x80u;
            const bool lead = (b & 0xC0) != 0x80;
            const uint64_t m = __ballot(lead);
            if (lead) {
                const uint32_t idx = cb + (uint32_t)__popcll(m & lt_mask);
                const uint32_t t1 = bi + 1 < nb ? txt[bi + 1] & 0x3Fu : 0u;
                const uint32_t t2 = bi + 2 < nb ? txt[bi + 2] & 0x3Fu : 0u;
                const uint32_t t3 = bi + 3 < nb ? txt[bi + 3] & 0x3Fu : 0u;
                uint32_t cp;
                if (b < 0x80) cp = b;
                else if (b < 0xE0) cp = ((b & 0x1F) << 6) | t1;
                else if (b < 0xF0) cp = ((b & 0x0F) << 12) | (t1 << 6) | t2;
                else cp = ((b & 0x07) << 18) | (t1 << 12) | (t2 << 6) | t3;
                ci[idx] = D.chr2inf[cp < 65536u ? cp : 0u];  // character.rs:112-116
                code[idx] = cp < D.sys.mapper_len ? D.sys.mapper[cp] : (uint16_t)0;
                if (D.has_user) ucode[idx] = cp < D.user.mapper_len ? D.user.mapper[cp] : (uint16_t)0;
                c2b[idx] = (IdxT)bi;
            }
            cb += (uint32_t)__popcll(m);
        }
        if (ln == 0) c2b[n] = (IdxT)nb;
    }
    __syncthreads();
    {   // groupable runs (Sentence::compute_groupable sentence.rs:57-71), right to left
        uint32_t carry = 0;
        for (int ch = (int)((n - 1) / 64); ch >= 0; --ch) {
            const uint32_t i = (uint32_t)ch * 64 + ln;
            const bool valid = i < n;
            bool link = false;
            if (valid && i + 1 < n) link = ((ci[i] & ci[i + 1]) & 0x3FFFFu) != 0;
            const uint64_t brk = __ballot(valid && !link);
            const uint64_t m = brk >> ln;
            const uint32_t g = m ? (uint32_t)__builtin_ctzll(m) + 1 : (64 - ln) + carry;
            if (valid) grp[i] = (IdxT)g;
            carry = (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
        }
    }
    __syncthreads();

    // ---- P1a: count candidates per start position ----
    uint32_t C = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += 64) {
        const uint32_t i = c0 + ln;
        uint32_t cnt = 0;
        if (i < n) {
            bool matched = false;
            if (D.has_user) matched |= walk_trie(D.user, ucode, i, n, [&](uint32_t, uint32_t c, uint32_t) { cnt += c; });
            matched |= walk_trie(D.sys, code, i, n, [&](uint32_t, uint32_t c, uint32_t) { cnt += c; });
            const uint32_t cinfo = ci[i], cate = (cinfo >> 18) & 0xFFu;
            const uint32_t nunk = D.unk_off[cate + 1] - D.unk_off[cate];
            unk_spans(cinfo, grp[i], i, matched, D.max_grouping_len, [&](uint32_t) { cnt += nunk; });
        }
        uint32_t tot;
        const uint32_t ex = wave_exscan(cnt, tot);
        if (i < n) cand_off[i] = (IdxT)(C + ex);
        if ((uint64_t)C + tot + 3 >= kIdxMax) return kNoFit;
        C += tot;
    }
    if (ln == 0) cand_off[n] = (IdxT)C;

    // start-major node arrays; node C is the EOS pseudo node (left id 0), C + 1 stands for BOS.  End-major: the lists.
    const uint64_t E = (uint64_t)C + 2;             // end-list slots: BOS in slot 0, EOS in slot C + 1
    uint64_t* lens = ar.take<uint64_t>(n + 1);      // per start position: bit L - 1 set <=> a candidate of length L
    StepRec<IdxT>* st;                              // sweep steps (one per visited start position, + EOS)
    if constexpr (sizeof(StepRec<IdxT>) == 8) st = reinterpret_cast<StepRec<IdxT>*>(lens);  // step S <= its start word: safe alias
    else st = ar.take<StepRec<IdxT>>(n + 1);
    double* e_alpha = ar.take<double>(E);           // per end-list slot: log weight of the paths BOS -> node (-inf: never reached)
    double* e_beta = ar.take<double>(E);            // ... of the paths node -> EOS (-inf: nothing follows it)
    uint32_t* nd_word = ar.take<uint32_t>(C);
    uint16_t* nd_left = ar.take<uint16_t>(C + 1);
    int16_t* nd_wcost = ar.take<int16_t>(C + 1);
    uint16_t* e_right = ar.take<uint16_t>(E);
    IdxT* nd_end = ar.take<IdxT>(C);
    IdxT* nd_eslot = ar.take<IdxT>(E);
    if (!ar.ok) return ar.used;
    uint16_t* tmp_right = reinterpret_cast<uint16_t*>(e_beta);  // right ids until the end lists exist (2 C <= 8 E bytes)

    for (uint32_t p = ln; p < n + 2; p += 64) end_off[p] = 0;
    for (uint32_t p = ln; p < n + 1; p += 64) reach[p] = 0;
    __syncthreads();

    // ---- P1b: fill candidates in reference insertion order (tokenizer.rs:155-198) ----
    bool any_long = false;  // a word longer than 64 chars: the windowed pre-pass cannot represent it
    for (uint32_t c0 = 0; c0 < n; c0 += 64) {
        const uint32_t i = c0 + ln;
        bool is_long = false;
        if (i < n) {
            uint32_t k = cand_off[i];
            uint64_t lmask = 0;
            bool matched = false;
            auto put = [&](const Entry* ent, uint32_t v, uint32_t c, uint32_t end, uint32_t lex) {
                const uint32_t len = end - i;
                if (len <= 64) lmask |= 1ull << (len - 1); else is_long = true;
                for (uint32_t t = 0; t < c; ++t, ++k) {
                    const Entry e = ent[v + t];
                    nd_word[k] = (lex << 30) | e.word_id;
                    nd_left[k] = (uint16_t)(e.left_right & 0xFFFFu);
                    tmp_right[k] = (uint16_t)(e.left_right >> 16);
                    nd_wcost[k] = (int16_t)(uint16_t)e.cost;
                    nd_end[k] = (IdxT)end;
                    nd_eslot[k] = (IdxT)atomicAdd(&end_off[end], 1u);  // slot within its end list (a sum does not care for the order)
                }
            };
            if (D.has_user)
                matched |= walk_trie(D.user, ucode, i, n, [&](uint32_t v, uint32_t c, uint32_t e) { put(D.user.entries, v, c, e, 1u); });
            matched |= walk_trie(D.sys, code, i, n, [&](uint32_t v, uint32_t c, uint32_t e) { put(D.sys.entries, v, c, e, 0u); });
            const uint32_t cinfo = ci[i], cate = (cinfo >> 18) & 0xFFu;
            const uint32_t u0 = D.unk_off[cate], nunk = D.unk_off[cate + 1] - u0;
            unk_spans(cinfo, grp[i], i, matched, D.max_grouping_len, [&](uint32_t e) { put(D.unk_entries, u0, nunk, e, 2u); });
            lens[i] = lmask;
        }
        any_long |= __ballot(is_long) != 0;
    }
    __syncthreads();

    // ---- P2: end lists: exclusive scan of the per-end counts; slot 0 is BOS (lattice.rs:72-83) ----
    {
        uint32_t running = 0;
        for (uint32_t c0 = 0; c0 < n + 1; c0 += 64) {
            const uint32_t p = c0 + ln;
            uint32_t cnt = 0;
            if (p < n + 1) cnt = load_counter<kGlobal>(&end_off[p]) + (p == 0 ? 1u : 0u);
            uint32_t tot;
            const uint32_t ex = wave_exscan(cnt, tot);
            if (p < n + 1) end_off[p] = running + ex;
            running += tot;
        }
        if (ln == 0) end_off[n + 1] = running;
    }
    __syncthreads();
    for (uint32_t c = ln; c < C; c += 64) {
        const uint32_t es = end_off[nd_end[c]] + nd_eslot[c];
        nd_eslot[c] = (IdxT)es;
        e_right[es] = tmp_right[c];
    }
    __syncthreads();  // all tmp_right reads done before beta is written
    for (uint64_t q = ln; q < E; q += 64) { e_alpha[q] = kNegInf; e_beta[q] = kNegInf; }
    __syncthreads();
    const uint32_t es_eos = C + 1;
    if (ln == 0) {
        e_right[0] = 0;  // BOS: right id 0, cost 0 (lattice.rs:72-83)
        e_alpha[0] = 0.0;
        nd_eslot[C + 1] = 0;
        nd_left[C] = 0;  // EOS: left id 0 (lattice.rs:85-101), no word cost
        nd_wcost[C] = 0;
        nd_eslot[C] = (IdxT)es_eos;
        e_beta[es_eos] = 0.0;
    }
    __syncthreads();

    // ---- P3a: structural pre-pass of build_lattice_inner (tokenizer.rs:106-138): one step record per visited start position + EOS ----
    uint32_t S = 0, sn_eos = 0;
    uint64_t total_pairs = 0, max_pairs = 0;
    bool windowed = !any_long;
    if (windowed) {
        U128 w{1, 0};  // bit b <=> a word ends at position p + b; BOS ends at position 0
        uint32_t p = 0;
        while (p < n) {
            w.lo = uniform64(w.lo);
            w.hi = uniform64(w.hi);
            p = __builtin_amdgcn_readfirstlane(p);
            if (!(w.lo & 1)) {  // has_previous_node(p) is false: skip to the next reachable position
                uint32_t z = w.lo ? (uint32_t)__builtin_ctzll(w.lo) : 64u;
                if (z > n - p) z = n - p;
                w = shr128(w, z);
                p += z;
                continue;
            }
            uint32_t sw = p;
            if (D.space_cateset) {  // tokenizer.rs:117-125
                const uint32_t cs = __builtin_amdgcn_readfirstlane(ci[p]);
                if (cs & D.space_cateset) sw += __builtin_amdgcn_readfirstlane((uint32_t)grp[p]);
            }
            if (sw >= n) break;  // input ends with spaces, tokenizer.rs:128-130
            const uint32_t d = sw - p + 1;
            if (d > 64) { windowed = false; break; }  // a space run too long for the window: generic path
            const uint64_t lm = uniform64(lens[sw]);
            const uint32_t c_beg = __builtin_amdgcn_readfirstlane((uint32_t)cand_off[sw]);
            const uint32_t c_end = __builtin_amdgcn_readfirstlane((uint32_t)cand_off[sw + 1]);
            const uint32_t p_beg = __builtin_amdgcn_readfirstlane(end_off[p]);
            const uint32_t p_end = __builtin_amdgcn_readfirstlane(end_off[p + 1]);
            if (ln == 0) st[S] = StepRec<IdxT>{(IdxT)c_beg, (IdxT)(c_end - c_beg), (IdxT)p_beg, (IdxT)(p_end - p_beg)};
            const uint64_t pairs = (uint64_t)(c_end - c_beg) * (p_end - p_beg);
            total_pairs += pairs;
            max_pairs = pairs > max_pairs ? pairs : max_pairs;
            ++S;
            w = shr128(or_shl128(w, lm, d), d);
            p = sw + 1;
        }
        sn_eos = p < n ? p : n;
        if (!windowed) { S = 0; total_pairs = 0; max_pairs = 0; }
    }
    if (!windowed) {  // generic path: byte-per-position reachability
        __syncthreads();
        if (ln == 0) reach[0] = 1;
        __syncthreads();
        uint32_t sn = 0, sw = 0;
        while (sw < n) {
            if (!__builtin_amdgcn_readfirstlane(reach[sn])) {  // has_previous_node, lattice.rs:155-157
                sw += 1;
                sn = sw;
                continue;
            }
            if (D.space_cateset) {
                const uint32_t cs = __builtin_amdgcn_readfirstlane(ci[sn]);
                if (cs & D.space_cateset) sw += __builtin_amdgcn_readfirstlane((uint32_t)grp[sn]);
            }
            if (sw >= n) break;
            const uint32_t c_beg = __builtin_amdgcn_readfirstlane((uint32_t)cand_off[sw]);
            const uint32_t c_end = __builtin_amdgcn_readfirstlane((uint32_t)cand_off[sw + 1]);
            const uint32_t p_beg = __builtin_amdgcn_readfirstlane(end_off[sn]);
            const uint32_t p_end = __builtin_amdgcn_readfirstlane(end_off[sn + 1]);
            for (uint32_t c = c_beg + ln; c < c_end; c += 64) reach[nd_end[c]] = 1;
            __syncthreads();  // (also orders the lens[] reads of other lanes before st[] overwrites them)
            if (ln == 0) st[S] = StepRec<IdxT>{(IdxT)c_beg, (IdxT)(c_end - c_beg), (IdxT)p_beg, (IdxT)(p_end - p_beg)};
            const uint64_t pairs = (uint64_t)(c_end - c_beg) * (p_end - p_beg);
            total_pairs += pairs;
            max_pairs = pairs > max_pairs ? pairs : max_pairs;
            ++S;
            sw += 1;
            sn = sw;
        }
        sn_eos = sn;
    }
    if (S == 0) { nothing(); return 0; }  // no position was visited: spaces only under ignore_space
    {   // EOS step (insert_eos(start_node), tokenizer.rs:138): one candidate (node C), predecessors = ends[sn]
        const uint32_t p_beg = __builtin_amdgcn_readfirstlane(end_off[sn_eos]);
        const uint32_t p_end = __builtin_amdgcn_readfirstlane(end_off[sn_eos + 1]);
        if (ln == 0) st[S] = StepRec<IdxT>{(IdxT)C, (IdxT)1, (IdxT)p_beg, (IdxT)(p_end - p_beg)};
        total_pairs += p_end - p_beg;
        max_pairs = (uint64_t)(p_end - p_beg) > max_pairs ? (uint64_t)(p_end - p_beg) : max_pairs;
        ++S;
    }
    // connection-cost staging: one cell per (candidate, predecessor) pair, read by both sweeps; all pairs if they fit (the backward
    // sweep then gathers nothing), else as many whole steps as fit (M.stage_cells: a cap of the staging for tests, 0 = none)
    uint64_t q_cap;
    ConnT* conn;
    {
        const uint64_t off = (ar.used + sizeof(ConnT) - 1) & ~(uint64_t)(sizeof(ConnT) - 1);
        uint64_t room = ar.cap > off ? (ar.cap - off) / sizeof(ConnT) : 0;
        if (room < max_pairs) return off + sizeof(ConnT) * max_pairs;
        if (M.stage_cells && room > M.stage_cells) room = M.stage_cells > max_pairs ? M.stage_cells : max_pairs;
        q_cap = room < total_pairs ? room : total_pairs;
        if (q_cap > 0xFFFFFFFFull) q_cap = 0xFFFFFFFFull;
        conn = reinterpret_cast<ConnT*>(ar.base + off);
    }
    __syncthreads();

    const ConnT* __restrict__ matrix = reinterpret_cast<const ConnT*>(D.matrix);
    const uint32_t NR = D.num_right;
    const uint32_t row = ln >> 4, l = ln & (kRowLanes - 1);
    const double nit = M.neg_inv_t;  // -1 / T
    auto step_pairs = [&](uint32_t kk) {
        const StepRec<IdxT> r = st[kk];
        return (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)r.nc) * __builtin_amdgcn_readfirstlane((uint32_t)r.np);
    };
    // the connection costs of the steps [k, kend) into conn[soff + j * nc + ci], soff = pairs of the block's steps before (consecutive
    // lanes = consecutive candidates); a slot is 64 consecutive pairs of one step, the (j, ci) of a lane advances by (64 / nc, 64 % nc)
    // from slot to slot: one division per step, none per pair; 16 gathers in flight
    auto gather = [&](uint32_t k, uint32_t kend) {
        constexpr int U = 16;
        uint32_t kk = k, q0 = 0, soff = 0;
        uint32_t c_beg = 0, nc = 1, p_beg = 0, pairs = 0, dq = 0, dr = 0;
        uint32_t pj = 0, pr = 0;
        auto load_step = [&]() {
            const StepRec<IdxT> r = st[kk];
            c_beg = __builtin_amdgcn_readfirstlane((uint32_t)r.cbeg);
            nc = __builtin_amdgcn_readfirstlane((uint32_t)r.nc);
            p_beg = __builtin_amdgcn_readfirstlane((uint32_t)r.pbeg);
            pairs = nc * __builtin_amdgcn_readfirstlane((uint32_t)r.np);
            dq = 64u / nc;
            dr = 64u - dq * nc;
            pj = ln / nc;
            pr = ln - pj * nc;
        };
        load_step();
        while (kk < kend) {
            int32_t val[U];
            uint32_t idx[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {  // U independent gathers before the first use; inactive slots re-read a valid cell
                kk = __builtin_amdgcn_readfirstlane(kk);
                q0 = __builtin_amdgcn_readfirstlane(q0);
                soff = __builtin_amdgcn_readfirstlane(soff);
                const bool live = kk < kend;
                const uint32_t ql = q0 + ln;
                const bool valid = live && ql < pairs;
                const uint32_t left = nd_left[c_beg + (valid ? pr : 0u)];
                const uint32_t right = e_right[p_beg + (valid ? pj : 0u)];
                val[u] = matrix[(size_t)left * NR + right];  // matrix_connector.rs:79-85
                idx[u] = valid ? soff + ql : 0xFFFFFFFFu;
                if (live) {
                    q0 += 64;
                    if (q0 >= pairs) {
                        soff += pairs;
                        q0 = 0;
                        ++kk;
                        if (kk < kend) load_step();
                    } else {
                        pj += dq;
                        pr += dr;
                        if (pr >= nc) { pr -= nc; ++pj; }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (idx[u] != 0xFFFFFFFFu) conn[idx[u]] = (ConnT)val[u];
        }
    };

    // ---- P4: forward.  alpha_c = -w_c / T + LSE_j(alpha_j - conn(j, c) / T): a candidate gets a ROW of 16 lanes (four candidates
    // per wave pass), lane l of the row walks the predecessors j = l (mod 16) with a running pair ----
    uint32_t st_lo = 0, st_hi = 0;  // the steps whose cells the staging holds
    for (uint32_t k = 0; k < S;) {
        uint32_t kend = k;
        for (uint64_t q = 0; kend < S; ++kend) {
            const uint64_t pairs = step_pairs(kend);
            if (q + pairs > q_cap) break;
            q += pairs;
        }
        gather(k, kend);
        st_lo = k; st_hi = kend;
        __syncthreads();
        uint32_t soff = 0;
        for (uint32_t kk = k; kk < kend; ++kk) {
            const StepRec<IdxT> sr = st[kk];
            const uint32_t c_beg = __builtin_amdgcn_readfirstlane((uint32_t)sr.cbeg);
            const uint32_t nc = __builtin_amdgcn_readfirstlane((uint32_t)sr.nc);
            const uint32_t p_beg = __builtin_amdgcn_readfirstlane((uint32_t)sr.pbeg);
            const uint32_t np = __builtin_amdgcn_readfirstlane((uint32_t)sr.np);
            for (uint32_t cb = 0; cb < nc; cb += kRows) {
                const uint32_t ci_ = cb + row;
                const bool live_row = ci_ < nc;
                const uint32_t c = c_beg + (live_row ? ci_ : 0u);
                const ConnT* col = conn + soff + (live_row ? ci_ : 0u);
                double m = kNegInf, s = 0.0;
                if (live_row)
                    for (uint32_t j = l; j < np; j += kRowLanes) {
                        const double a = e_alpha[p_beg + j];
                        if (a != kNegInf) lse_add(m, s, a + (double)col[(size_t)j * nc] * nit);
                    }
                row_lse(m, s);
                if (live_row && l == 0) e_alpha[nd_eslot[c]] = s > 0.0 ? (double)nd_wcost[c] * nit + (m + log(s)) : kNegInf;
            }
            soff += nc * np;
            __syncthreads();
        }
        k = kend;
    }

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
