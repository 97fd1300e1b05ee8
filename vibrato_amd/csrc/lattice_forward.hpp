// The float64 forward sweep over a sentence's lattice, shared by marginal.hip (forward-backward) and sample.hip
// (forward filtering / backward sampling, 3.4h): phases P0-P3a, the connection-cost gather and P4, one wavefront per sentence.  It
// leaves alpha -- the log of the summed weight exp(-cost / T) of the partial paths from BOS that end in a node, the node's own word
// cost included -- for every end-list slot of the arena, and hands over to the `tail` of the kernel that instantiates it.
//
// Forward: the step records in order, a candidate owns a row of 16 lanes, the lanes stride its predecessors.  Every lane keeps a
// running (maximum, sum of exp(x - maximum)) pair, the 16 pairs of a row are combined with four DPP steps on the two halves of the
// doubles; a step of any size needs no other state.  Costs are exact: int16 / int32 cells and int16 word costs go to float64 one
// by one, nothing is summed in i32, so nothing wraps.
//
// A tail is a struct with
//   static constexpr bool kBeta          the aux region is beta[E] (initialised to -inf, 0 for EOS)
//   static constexpr bool kOrderedLists  end-list slots in node order (= the reference's insertion order) instead of the order the
//                                        atomics hand out, and e_node[slot] = the node of a slot (C + 1 for BOS)
//   uint64_t aux_bytes(n, C, E)          bytes of the aux region (>= 2 C: the right ids live there until the end lists exist)
//   void none(bool spaces_only)          the sentence has no lattice: it is empty, or every character is a skipped space
//   uint64_t run(X, gather, step_pairs)  everything behind P4; X is the FwdCtx below
#pragma once
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

// What the forward sweep leaves for the tail: the arena's arrays (start-major node arrays nd_*, end-major e_*), the step records
// and the state of the connection-cost staging (conn holds the cells of the steps [st_lo, st_hi), q_cap cells at most).
template <typename IdxT, typename ConnT>
struct FwdCtx {
    uint32_t n, C, S, es_eos;
    const IdxT *c2b, *cand_off, *nd_end, *nd_eslot, *e_node;
    const StepRec<IdxT>* st;
    double* e_alpha;
    void* aux;
    const uint32_t* nd_word;
    const uint16_t *nd_left, *e_right;
    const int16_t* nd_wcost;
    ConnT* conn;
    const ConnT* matrix;
    uint32_t NR;
    uint64_t q_cap;
    uint32_t st_lo, st_hi;
    double nit;  // -1 / T
};

// The forward sweep of sentence `sid` inside the arena [abase, abase + acap), then tail.run().  Returns 0 when done, otherwise the
// arena bytes it would need (kNoFit: never in this tier).  Phases P0-P3a are those of fused.hip's process_sentence (decode,
// character classes, trie walks, unknown words, candidates in reference insertion order, end lists, step records) with this
// kernel's node layout.  neg_inv_t = -1 / T; stage_cells: a cap of the connection-cost staging in cells (0 = none).
template <typename IdxT, bool kGlobal, bool kWide, typename Tail>
__device__ __forceinline__ uint64_t forward_sentence(const DevDict& D, const BatchArgs& A, double neg_inv_t, uint32_t stage_cells, uint32_t sid, char* abase,
                                                     uint64_t acap, const Tail& tail) {
    typedef typename std::conditional<kWide, int32_t, int16_t>::type ConnT;
    const uint32_t ln = threadIdx.x;
    const uint64_t lt_mask = (1ull << ln) - 1ull;
    constexpr uint64_t kIdxMax = sizeof(IdxT) == 2 ? 0xFFFFull : 0xFFFFFFF0ull;
    const uint64_t b0 = A.offsets[sid], nb64 = A.offsets[sid + 1] - b0;
    if (nb64 == 0) { tail.none(false); return 0; }  // an empty sentence (worker.rs:50-52)
    if (nb64 >= (sizeof(IdxT) == 2 ? 0xFFFFull : 0xFFFFFFFFull)) return kNoFit;
    const uint32_t nb = (uint32_t)nb64;
    const uint8_t* __restrict__ txt = A.text + b0;
    const uint32_t n = count_chars(txt, nb);
    if (n == 0) { tail.none(false); return 0; }

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
    double* aux = ar.take<double>((tail.aux_bytes(n, C, E) + 7) / 8);  // the tail's: beta per slot (marginals), the walk state (samples)
    uint32_t* nd_word = ar.take<uint32_t>(C);
    uint16_t* nd_left = ar.take<uint16_t>(C + 1);
    int16_t* nd_wcost = ar.take<int16_t>(C + 1);
    uint16_t* e_right = ar.take<uint16_t>(E);
    IdxT* nd_end = ar.take<IdxT>(C);
    IdxT* nd_eslot = ar.take<IdxT>(E);
    IdxT* e_node = nullptr;                         // the node in an end-list slot
    if constexpr (Tail::kOrderedLists) e_node = ar.take<IdxT>(E);
    if (!ar.ok) return ar.used;
    uint16_t* tmp_right = reinterpret_cast<uint16_t*>(aux);  // right ids until the end lists exist (2 C <= aux bytes)

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
                    if constexpr (!Tail::kOrderedLists) nd_eslot[k] = (IdxT)atomicAdd(&end_off[end], 1u);  // slot within its end list (a sum does not care for the order)
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
    if constexpr (Tail::kOrderedLists) {
        // slot of node c within its end list = the nodes below c with the same end: the reference's insertion order (lattice.rs:103-151
        // pushes in lattice order).  64 nodes at a time; the lanes that share an end position take consecutive slots behind its count.
        for (uint32_t c0 = 0; c0 < C; c0 += 64) {
            const uint32_t c = c0 + ln;
            const bool valid = c < C;
            const uint32_t en = valid ? (uint32_t)nd_end[c] : 0xFFFFFFFFu;
            uint64_t todo = __ballot(valid);
            while (todo) {
                const uint32_t e = (uint32_t)__shfl((int)en, (int)__builtin_ctzll(todo));
                const uint64_t m = __ballot(en == e);
                const uint32_t have = end_off[e];
                if (en == e) nd_eslot[c] = (IdxT)(have + (uint32_t)__popcll(m & lt_mask));
                if (ln == (uint32_t)__builtin_ctzll(m)) end_off[e] = have + (uint32_t)__popcll(m);
                todo &= ~m;
            }
            __syncthreads();
        }
    }

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
        if constexpr (Tail::kOrderedLists) e_node[es] = (IdxT)c;
    }
    __syncthreads();  // all tmp_right reads done before the aux region is written
    for (uint64_t q = ln; q < E; q += 64) {
        e_alpha[q] = kNegInf;
        if constexpr (Tail::kBeta) aux[q] = kNegInf;
    }
    __syncthreads();
    const uint32_t es_eos = C + 1;
    if (ln == 0) {
        e_right[0] = 0;  // BOS: right id 0, cost 0 (lattice.rs:72-83)
        e_alpha[0] = 0.0;
        nd_eslot[C + 1] = 0;
        nd_left[C] = 0;  // EOS: left id 0 (lattice.rs:85-101), no word cost
        nd_wcost[C] = 0;
        nd_eslot[C] = (IdxT)es_eos;
        if constexpr (Tail::kBeta) aux[es_eos] = 0.0;
        if constexpr (Tail::kOrderedLists) { e_node[0] = (IdxT)(C + 1); e_node[es_eos] = (IdxT)C; }
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
    if (S == 0) { tail.none(true); return 0; }  // no position was visited: spaces only under ignore_space
    {   // EOS step (insert_eos(start_node), tokenizer.rs:138): one candidate (node C), predecessors = ends[sn]
        const uint32_t p_beg = __builtin_amdgcn_readfirstlane(end_off[sn_eos]);
        const uint32_t p_end = __builtin_amdgcn_readfirstlane(end_off[sn_eos + 1]);
        if (ln == 0) st[S] = StepRec<IdxT>{(IdxT)C, (IdxT)1, (IdxT)p_beg, (IdxT)(p_end - p_beg)};
        total_pairs += p_end - p_beg;
        max_pairs = (uint64_t)(p_end - p_beg) > max_pairs ? (uint64_t)(p_end - p_beg) : max_pairs;
        ++S;
    }
    // connection-cost staging: one cell per (candidate, predecessor) pair, read by both sweeps; all pairs if they fit (the backward
    // sweep then gathers nothing), else as many whole steps as fit (stage_cells: a cap of the staging for tests, 0 = none)
    uint64_t q_cap;
    ConnT* conn;
    {
        const uint64_t off = (ar.used + sizeof(ConnT) - 1) & ~(uint64_t)(sizeof(ConnT) - 1);
        uint64_t room = ar.cap > off ? (ar.cap - off) / sizeof(ConnT) : 0;
        if (room < max_pairs) return off + sizeof(ConnT) * max_pairs;
        if (stage_cells && room > stage_cells) room = stage_cells > max_pairs ? stage_cells : max_pairs;
        q_cap = room < total_pairs ? room : total_pairs;
        if (q_cap > 0xFFFFFFFFull) q_cap = 0xFFFFFFFFull;
        conn = reinterpret_cast<ConnT*>(ar.base + off);
    }
    __syncthreads();

    const ConnT* __restrict__ matrix = reinterpret_cast<const ConnT*>(D.matrix);
    const uint32_t NR = D.num_right;
    const uint32_t row = ln >> 4, l = ln & (kRowLanes - 1);
    const double nit = neg_inv_t;  // -1 / T
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

    FwdCtx<IdxT, ConnT> X{n, C, S, es_eos, c2b, cand_off, nd_end, nd_eslot, e_node, st, e_alpha, aux, nd_word, nd_left, e_right, nd_wcost,
                          conn, matrix, NR, q_cap, st_lo, st_hi, nit};
    return tail.run(X, gather, step_pairs);
}

}  // namespace
}  // namespace vbt
