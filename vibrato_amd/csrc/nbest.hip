// N-best tokenization (MeCab's -N): the K cheapest paths through the lattice the 1-best path is taken from,
// one wavefront per sentence, in a translation unit of its own (nothing shared with lattice.hip / fused.hip but device_common.hpp).
// The sweep of Lattice::insert_node / search_min_node (lattice.rs:103-151) keeps ONE (min_cost, back pointer) per node; here every
// node keeps its K best partial paths, sorted, and a candidate's list is the K-way merge of its predecessors' lists, each shifted
// by the connection cost of the pair.
//
// Order (total, so results are reproducible): lower cost first; on equal cost the paths are compared from EOS backwards and at
// the first node where they differ -- two nodes of one end list -- the node inserted LATER comes first: the `<=` of
// search_min_node (lattice.rs:141-146) applied recursively, so rank 0 is the path of the 1-best sweep.  Restricted to the partial
// paths that end in one node this is (cost so far, predecessor inserted later first, lower rank of the predecessor's entry first),
// which one unsigned 64-bit comparison decides on the keys below; it is monotone under extension, so K entries per node suffice.
//
// Entry = 8-byte key {cost ^ 0x80000000, (0x0FFFFFFE - sequence number of the node) << 4 | rank} + 4-byte back reference = the
// low word of the predecessor entry's key (its node and rank).  A predecessor's key + (connection cost << 32) is the OFFER the
// merge compares: its low word is exactly the tie-break, and it becomes the back reference of the entry it wins.
#include "device_common.hpp"

namespace vbt {
namespace {

constexpr uint32_t kSeqTop = 0x0FFFFFFEu;  // 28-bit sequence numbers: candidates 0 .. C - 1, EOS = C, BOS = C + 1
__device__ __forceinline__ uint64_t nb_key(uint32_t cost, uint32_t seq, uint32_t rank) {
    return ((uint64_t)(cost ^ 0x80000000u) << 32) | ((kSeqTop - seq) << 4) | rank;
}
__device__ __forceinline__ bool nb_dead(uint64_t k) { return (uint32_t)k == 0xFFFFFFFFu; }
__device__ __forceinline__ uint32_t ref_seq(uint32_t ref) { return kSeqTop - (ref >> 4); }
__device__ __forceinline__ uint32_t ref_rank(uint32_t ref) { return ref & 15u; }

// Minimum of a 64-bit key over the 16 lanes of a DPP row, left in every lane of the row: four DPP steps (the two quad permutes,
// row_half_mirror, row_mirror), no LDS traffic.  Every lane of the wave must be active.
template <int kCtrl>
__device__ __forceinline__ uint64_t dpp_min_u64(uint64_t x) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)x, kCtrl, 0xF, 0xF, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(x >> 32), kCtrl, 0xF, 0xF, true);
    const uint64_t o = ((uint64_t)hi << 32) | lo;
    return o < x ? o : x;
}
__device__ __forceinline__ uint64_t row_min_u64(uint64_t x) {
    x = dpp_min_u64<0xB1>(x);
    x = dpp_min_u64<0x4E>(x);
    x = dpp_min_u64<0x141>(x);
    x = dpp_min_u64<0x140>(x);
    return x;
}

constexpr uint32_t kRowLanes = 16, kRows = 4, kChunkPreds = 256;  // a row owns 16 x 16 predecessor heads (4 bits each in one u64)

// The K best paths of sentence `sid` inside the arena [abase, abase + acap).  Returns 0 when done, otherwise the arena bytes it
// would need (kNoFit: never in this tier).  Phases P0-P3a are those of fused.hip's process_sentence (decode, character classes,
// trie walks, unknown words, candidates in reference insertion order, end lists, step records) with this kernel's node layout.
template <typename IdxT, bool kGlobal, bool kWide>
__device__ __forceinline__ uint64_t nbest_sentence(const DevDict& D, const BatchArgs& A, const NBestArgs& NB, uint32_t sid, char* abase, uint64_t acap) {
    typedef typename std::conditional<kWide, int32_t, int16_t>::type ConnT;
    const uint32_t ln = threadIdx.x, K = NB.k;
    const uint64_t lt_mask = (1ull << ln) - 1ull;
    constexpr uint64_t kIdxMax = sizeof(IdxT) == 2 ? 0xFFFFull : (uint64_t)kSeqTop;
    const uint64_t b0 = A.offsets[sid], nb64 = A.offsets[sid + 1] - b0;
    if (nb64 == 0) {  // nothing is computed for an empty sentence (worker.rs:50-52): no paths
        if (ln == 0) A.tok_cnt[sid] = 0;
        return 0;
    }
    if (nb64 >= (sizeof(IdxT) == 2 ? 0xFFFFull : 0xFFFFFFFFull)) return kNoFit;
    const uint32_t nb = (uint32_t)nb64;
    const uint8_t* __restrict__ txt = A.text + b0;
    const uint32_t n = count_chars(txt, nb);
    if (n == 0) {
        if (ln == 0) A.tok_cnt[sid] = 0;
        return 0;
    }

    Arena ar{abase, acap, 0, true};
    uint32_t* ci = ar.take<uint32_t>(n);            // CharInfo per char
    uint32_t* end_off = ar.take<uint32_t>(n + 2);   // end-list offsets
    uint16_t* code = ar.take<uint16_t>(n);          // system-trie code per char
    uint16_t* ucode = D.has_user ? ar.take<uint16_t>(n) : code;
    IdxT* c2b = ar.take<IdxT>(n + 1);               // char -> byte offset
    IdxT* grp = ar.take<IdxT>(n);                   // groupable run length
    IdxT* cand_off = ar.take<IdxT>(n + 1);          // candidates by start position (CSR)
    uint8_t* reach = ar.take<uint8_t>(n + 1);       // has_previous_node
    if (!ar.ok) return ar.used + (uint64_t)n * 64 * K;  // lower bound; the exact size follows after counting

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
    uint64_t* e_key = ar.take<uint64_t>(E * K);     // K sorted keys per end-list slot (kDeadKey: unused)
    uint32_t* e_back = ar.take<uint32_t>(E * K);    // their back references
    uint32_t* nd_word = ar.take<uint32_t>(C);
    uint16_t* nd_left = ar.take<uint16_t>(C + 1);
    int16_t* nd_wcost = ar.take<int16_t>(C + 1);
    uint16_t* e_right = ar.take<uint16_t>(E);
    IdxT* nd_end = ar.take<IdxT>(C);
    IdxT* nd_eslot = ar.take<IdxT>(E);
    if (!ar.ok) return ar.used;
    uint16_t* tmp_right = reinterpret_cast<uint16_t*>(e_back);  // right ids until the end lists exist (2 C <= 4 E K bytes)

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
                    nd_eslot[k] = (IdxT)atomicAdd(&end_off[end], 1u);  // slot within its end list (order irrelevant: the keys carry the sequence numbers)
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
    __syncthreads();  // all tmp_right reads done before the lists are written
    for (uint64_t q = ln; q < E * K; q += 64) e_key[q] = kDeadKey;  // nothing inserted until a step reaches the node's start position
    __syncthreads();
    const uint32_t kBosSeq = C + 1, es_eos = C + 1;
    if (ln == 0) {
        e_right[0] = 0;  // BOS: right id 0, cost 0 (lattice.rs:72-83): one entry
        e_key[0] = nb_key(0u, kBosSeq, 0u);
        e_back[0] = 0;
        nd_eslot[kBosSeq] = 0;
        nd_left[C] = 0;  // EOS: left id 0 (lattice.rs:85-101), no word cost
        nd_wcost[C] = 0;
        nd_eslot[C] = (IdxT)es_eos;
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
    {   // EOS step (insert_eos(start_node), tokenizer.rs:138): one candidate (node C), predecessors = ends[sn]
        const uint32_t p_beg = __builtin_amdgcn_readfirstlane(end_off[sn_eos]);
        const uint32_t p_end = __builtin_amdgcn_readfirstlane(end_off[sn_eos + 1]);
        if (ln == 0) st[S] = StepRec<IdxT>{(IdxT)C, (IdxT)1, (IdxT)p_beg, (IdxT)(p_end - p_beg)};
        total_pairs += p_end - p_beg;
        max_pairs = (uint64_t)(p_end - p_beg) > max_pairs ? (uint64_t)(p_end - p_beg) : max_pairs;
        ++S;
    }
    // connection-cost staging: ONE cell per (candidate, predecessor) pair -- the K ranks of a predecessor share it; all pairs if
    // they fit, else as many whole steps as fit
    uint64_t q_cap;
    ConnT* conn;
    {
        const uint64_t off = (ar.used + sizeof(ConnT) - 1) & ~(uint64_t)(sizeof(ConnT) - 1);
        const uint64_t room = ar.cap > off ? (ar.cap - off) / sizeof(ConnT) : 0;
        if (room < max_pairs) return off + sizeof(ConnT) * max_pairs;
        q_cap = room < total_pairs ? room : total_pairs;
        if (q_cap > 0xFFFFFFFFull) q_cap = 0xFFFFFFFFull;
        conn = reinterpret_cast<ConnT*>(ar.base + off);
    }
    __syncthreads();

    // ---- P3b / P4: per block of steps: gather the connection costs with many loads in flight, then the merges ----
    const ConnT* __restrict__ matrix = reinterpret_cast<const ConnT*>(D.matrix);
    const uint32_t NR = D.num_right;
    const uint32_t row = ln >> 4, l = ln & (kRowLanes - 1);
    for (uint32_t k = 0; k < S;) {
        uint32_t kend = k;
        {
            uint64_t q = 0;
            while (kend < S) {
                const StepRec<IdxT> r = st[kend];
                const uint64_t pairs = (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)r.nc) * __builtin_amdgcn_readfirstlane((uint32_t)r.np);
                if (q + pairs > q_cap) break;
                q += pairs;
                ++kend;
            }
        }
        {   // gather: conn[soff + j * nc + ci] (consecutive lanes = consecutive candidates); a slot is 64 consecutive pairs of one
            // step, the (j, ci) of a lane advances by (64 / nc, 64 % nc) from slot to slot: one division per step, none per pair
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
        }
        __syncthreads();
        // The merges.  A candidate gets a ROW of 16 lanes (four candidates per wave pass); lane l of the row owns the predecessors
        // j = l (mod 16) of the current chunk of 256 and keeps a 4-bit head rank for each in one 64-bit register.  Each round every
        // lane offers the smallest key among its heads, the row takes the minimum (DPP), the winning lane advances that head and
        // lane r of the row keeps the winner as the candidate's entry r.  K rounds, or until the row minimum is dead.  A step with
        // more than 256 predecessors runs chunk by chunk, the candidate's own list (as offers) being one more source of lane 0.
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
                uint64_t* own = e_key + (size_t)nd_eslot[c] * K;
                const ConnT* col = conn + soff + (live_row ? ci_ : 0u);
                uint64_t out = kDeadKey;  // this lane's entry (rank l) of the candidate's list, as an offer
                for (uint32_t jb = 0; jb < np; jb += kChunkPreds) {
                    const uint32_t npc = np - jb < kChunkPreds ? np - jb : kChunkPreds;
                    uint64_t hd = 0, offer = kDeadKey;
                    uint32_t offer_t = 0, ownh = 0;
                    bool stale = live_row;
                    out = kDeadKey;
                    for (uint32_t r = 0; r < K; ++r) {
                        if (stale) {  // this lane's offer: the smallest key among the heads it owns
                            offer = kDeadKey;
                            for (uint32_t t = 0, jj = l; jj < npc; ++t, jj += kRowLanes) {
                                const uint32_t j = jb + jj, h = (uint32_t)(hd >> (4 * t)) & 15u;
                                if (h >= K) continue;  // (a head reaches K only with the last round: never read again)
                                const uint64_t pk = e_key[(size_t)(p_beg + j) * K + h];
                                const uint32_t cv = (uint32_t)(int32_t)col[(size_t)j * nc];
                                const uint64_t ok = nb_dead(pk) ? kDeadKey : pk + ((uint64_t)cv << 32);  // wrapping i32 add of the connection cost
                                if (ok < offer) { offer = ok; offer_t = t; }
                            }
                            if (jb > 0 && l == 0 && ownh < K) {
                                const uint64_t ok = own[ownh];
                                if (ok < offer) { offer = ok; offer_t = 16; }
                            }
                            stale = false;
                        }
                        const uint64_t best = row_min_u64(offer);
                        if (__ballot(!nb_dead(best)) == 0) break;  // every row of the wave is exhausted
                        if (!nb_dead(best) && offer == best) {     // offers are distinct (node, rank): one winner per row
                            if (offer_t == 16) ++ownh; else hd += 1ull << (4 * offer_t);
                            stale = true;
                        }
                        if (l == r) out = best;
                    }
                    if (np > kChunkPreds) {  // the list so far becomes a source of the next chunk
                        __syncthreads();
                        if (live_row && l < K) own[l] = out;
                        __syncthreads();
                    }
                }
                if (live_row && l < K) {  // lattice.rs:125: + word cost; the entry's own key names this node and rank
                    const uint32_t wcost = (uint32_t)(int32_t)nd_wcost[c];
                    own[l] = nb_dead(out) ? kDeadKey : nb_key(key_cost(out) + wcost, c, l);
                    e_back[(size_t)nd_eslot[c] * K + l] = (uint32_t)out;
                }
            }
            soff += nc * np;
            __syncthreads();
        }
        k = kend;
    }

    // ---- P5: EOS's list holds the paths; lane r traces path r through the back references (append_top_nodes lattice.rs:159-168) ----
    uint32_t T = 0;
    uint64_t pkey = kDeadKey;
    if (ln < K) pkey = e_key[(size_t)es_eos * K + ln];
    const bool has_path = !nb_dead(pkey);
    if (has_path) {
        uint32_t ref = e_back[(size_t)es_eos * K + ln];
        while (ref_seq(ref) != kBosSeq && T < n) {  // tokens <= chars; the bound also keeps a corrupted chain finite
            ++T;
            ref = e_back[(size_t)nd_eslot[ref_seq(ref)] * K + ref_rank(ref)];
        }
    }
    const uint32_t P = (uint32_t)__popcll(__ballot(has_path));
    if (ln == 0) A.tok_cnt[sid] = P;
    if (ln < K) {
        NB.path_cnt[(size_t)sid * K + ln] = T;
        NB.path_cost[(size_t)sid * K + ln] = has_path ? (int32_t)key_cost(pkey) : 0;
    }
    // records: path r of the sentence owns nb + kSentenceSlack slots of the sentence's staging region (tokens <= characters <= bytes),
    // in reference token order (Worker::token: index = n - 1 - i, worker.rs:65-68)
    if (has_path) {
        vbt_token_rec* outp = NB.stage + sentence_slot(A, b0, sid) * K + (size_t)ln * (nb + kSentenceSlack);
        uint32_t ref = e_back[(size_t)es_eos * K + ln];
        for (uint32_t t = 0; t < T; ++t) {
            const uint32_t c = ref_seq(ref);
            const size_t e = (size_t)nd_eslot[c] * K + ref_rank(ref);
            uint32_t lo = 0, hi = n;  // start_word = the position whose candidate range contains c
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if ((uint32_t)cand_off[mid + 1] <= c) lo = mid + 1; else hi = mid;
            }
            const uint32_t en = nd_end[c];
            vbt_token_rec r;
            r.start_char = lo; r.end_char = en;
            r.start_byte = c2b[lo]; r.end_byte = c2b[en];
            r.word_idx = nd_word[c];
            r.total_cost = (int32_t)key_cost(e_key[e]);  // the cost accumulated along THIS path
            outp[T - 1 - t] = r;
            ref = e_back[e];
        }
    }
    return 0;
}

// LDS tier: one wavefront per sentence (block b = sentence b), the arena in `lds_bytes` of dynamic LDS; what does not fit is
// filed for the slab tier.
template <bool kWide>
__global__ void __launch_bounds__(64) nbest_lds(DevDict D, BatchArgs A, NBestArgs NB, uint32_t lds_bytes, uint32_t* out_list, uint32_t* out_count) {
    if (batch_rejected(A)) return;
    const uint32_t sid = blockIdx.x;
    if (nbest_sentence<uint16_t, false, kWide>(D, A, NB, sid, g_smem, lds_bytes) != 0 && threadIdx.x == 0) out_list[atomicAdd(out_count, 1u)] = sid;
}

// Slab tier: persistent waves, the arena in a private slab of global memory taken from the scratch bump allocator (any length).
template <bool kWide>
__global__ void __launch_bounds__(64) nbest_slab(DevDict D, BatchArgs A, NBestArgs NB, const uint32_t* in_list, const uint32_t* in_count, uint32_t* cursor) {
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
            const uint64_t need = nbest_sentence<uint32_t, true, kWide>(D, A, NB, sid, slab, slab_bytes);
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
                }
                break;
            }
            __syncthreads();
        }
        __syncthreads();
    }
}

// ---- pack pass: (sentence, rank) is a row; row i = s * K + r exists when r < paths[s].  Tiles of 256 rows.
constexpr uint32_t kPackTile = 256;
__device__ __forceinline__ void pack_row(const BatchArgs& A, const NBestArgs& NB, uint64_t i, uint32_t& exists, uint32_t& cnt) {
    exists = 0; cnt = 0;
    if (i < (uint64_t)A.n * NB.k) {
        const uint32_t s = (uint32_t)(i / NB.k), r = (uint32_t)(i - (uint64_t)s * NB.k);
        exists = r < A.tok_cnt[s] ? 1u : 0u;
        cnt = exists ? NB.path_cnt[i] : 0u;
    }
}
__global__ void __launch_bounds__(256) nbest_tile_sums(BatchArgs A, NBestArgs NB) {
    __shared__ uint32_t ws[4];
    uint32_t exists, cnt, tp, tt;
    pack_row(A, NB, (uint64_t)blockIdx.x * kPackTile + threadIdx.x, exists, cnt);
    block_exscan(exists, ws, tp);
    block_exscan(cnt, ws, tt);
    if (threadIdx.x == 0) { NB.tile_paths[blockIdx.x] = tp; NB.tile_toks[blockIdx.x] = tt; }
}
// one workgroup: exclusive prefix of the tiles' sums in place; totals[0] = paths, totals[1] = tokens, path_off[n], tok_off[paths]
__global__ void __launch_bounds__(256) nbest_tile_scan(BatchArgs A, NBestArgs NB, uint32_t n_tiles) {
    __shared__ uint32_t ws[4];
    uint32_t run_p = 0, run_t = 0;
    if (!batch_rejected(A))
        for (uint32_t t0 = 0; t0 < n_tiles; t0 += 256) {
            const uint32_t t = t0 + threadIdx.x;
            const uint32_t vp = t < n_tiles ? NB.tile_paths[t] : 0u, vt = t < n_tiles ? NB.tile_toks[t] : 0u;
            uint32_t tp, tt;
            const uint32_t ep = block_exscan(vp, ws, tp), et = block_exscan(vt, ws, tt);
            if (t < n_tiles) { NB.tile_paths[t] = run_p + ep; NB.tile_toks[t] = run_t + et; }
            run_p += tp; run_t += tt;
        }
    if (threadIdx.x == 0) {
        NB.totals[0] = run_p; NB.totals[1] = run_t;
        NB.path_off[A.n] = run_p;
        NB.tok_off[run_p] = run_t;
    }
}
// path_off[s], tok_off[p], path_cost[p] and the records, sentence-major, rank-minor
__global__ void __launch_bounds__(256) nbest_pack(BatchArgs A, NBestArgs NB) {
    __shared__ uint32_t ws[4];
    __shared__ uint64_t src[kPackTile];
    __shared__ uint32_t dst[kPackTile], num[kPackTile];
    if (batch_rejected(A)) return;
    const uint64_t i = (uint64_t)blockIdx.x * kPackTile + threadIdx.x;
    uint32_t exists, cnt, tot;
    pack_row(A, NB, i, exists, cnt);
    const uint32_t p = NB.tile_paths[blockIdx.x] + block_exscan(exists, ws, tot);
    const uint32_t q = NB.tile_toks[blockIdx.x] + block_exscan(cnt, ws, tot);
    num[threadIdx.x] = cnt;
    if (i < (uint64_t)A.n * NB.k) {
        const uint32_t s = (uint32_t)(i / NB.k), r = (uint32_t)(i - (uint64_t)s * NB.k);
        if (r == 0) NB.path_off[s] = p;
        if (exists) {
            NB.tok_off[p] = q;
            NB.path_cost_out[p] = NB.path_cost[i];
            const uint64_t o0 = A.offsets[0], b0 = A.offsets[s], nb = A.offsets[s + 1] - b0;
            src[threadIdx.x] = ((b0 - o0) + (uint64_t)kSentenceSlack * s) * NB.k + (uint64_t)r * (nb + kSentenceSlack);
            dst[threadIdx.x] = q;
        }
    }
    __syncthreads();
    // a wave per row, a dword per lane: records are 6 dwords
    for (uint32_t rw = threadIdx.x >> 6; rw < kPackTile; rw += 4) {
        const uint32_t words = num[rw] * 6u;
        if (!words) continue;
        const uint32_t* __restrict__ from = reinterpret_cast<const uint32_t*>(NB.stage + src[rw]);
        uint32_t* __restrict__ to = reinterpret_cast<uint32_t*>(NB.tokens + dst[rw]);
        for (uint32_t w = threadIdx.x & 63u; w < words; w += 64) to[w] = from[w];
    }
}

}  // namespace

namespace kern {

void nbest_lds(uint32_t n, uint32_t lds_bytes, hipStream_t stream, const DevDict& D, const BatchArgs& a, const NBestArgs& nb, uint32_t* out_list, uint32_t* out_count) {
    hipLaunchKernelGGL(D.matrix_wide ? vbt::nbest_lds<true> : vbt::nbest_lds<false>, dim3(n), dim3(64), lds_bytes, stream, D, a, nb, lds_bytes, out_list, out_count);
}
void nbest_slab(uint32_t workgroups, hipStream_t stream, const DevDict& D, const BatchArgs& a, const NBestArgs& nb, const uint32_t* in_list, const uint32_t* in_count, uint32_t* cursor) {
    hipLaunchKernelGGL(D.matrix_wide ? vbt::nbest_slab<true> : vbt::nbest_slab<false>, dim3(workgroups), dim3(64), 0, stream, D, a, nb, in_list, in_count, cursor);
}
void nbest_pack(hipStream_t stream, const BatchArgs& a, const NBestArgs& nb) {
    const uint32_t n_tiles = (uint32_t)(((uint64_t)a.n * nb.k + kPackTile - 1) / kPackTile);
    hipLaunchKernelGGL(vbt::nbest_tile_sums, dim3(n_tiles), dim3(256), 0, stream, a, nb);
    hipLaunchKernelGGL(vbt::nbest_tile_scan, dim3(1), dim3(256), 0, stream, a, nb, n_tiles);
    hipLaunchKernelGGL(vbt::nbest_pack, dim3(n_tiles), dim3(256), 0, stream, a, nb);
}

}  // namespace kern
}  // namespace vbt
