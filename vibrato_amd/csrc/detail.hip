// Detail output rendered on the device (tokenize/src/main.rs:108-123): per token
//     surface \t feature \tlex_type=System|User|Unknown \tleft_id=N \tright_id=N \tword_cost=N \ttotal_cost=N \n
// then "EOS\n"; "EOS\n" alone for a sentence without tokens.  mecab.hip's scheme with a longer piece table: behind its surface and
// its feature a token has a TAIL of 52 label bytes, the lexicon's name, four decimal fields and '\n' -- 62 to 87 bytes that exist
// nowhere in memory.  DESIGN.md section 3.4c.
//
// Where the numbers come from: total_cost is word 5 of the staged record, the lexicon the top two bits of word_idx; left_id,
// right_id and word_cost are read from DevWordParams, the DICTIONARY's ids (the entry arrays of a DevImage carry device ids, which
// the calibration renumbers).
//
// detail_plan (one workgroup per tile of kScanTile sentences): line_len[s] (u64) and the bytes of the tile; a field's width comes
// from compares against the powers of ten.
// text_tile_scan (wakati.hip, shared): the tiles' prefix, line_off[n] = the exact total, whatever the capacity.
// detail_render (one workgroup per tile): output-stationary as mecab_render -- a wave takes a round of up to kDetailRound tokens into
// an LDS piece table, every lane owns one ALIGNED dword of the round's span and finds the token of its first byte by binary search
// in the output starts; a dword inside one feature is two aligned dword loads and a byte-align.  The binary-to-decimal conversion
// happens ONCE per token, when the lane that loads token k fills the table: multiply-high by the reciprocal of ten, the digits kept
// as packed BCD next to the field widths.  A lane that produces a byte of a tail finds its field by five compares against the
// cumulative field ends and takes a label byte from a 72-byte string in LDS or '0' + a nibble: no division anywhere, no load from
// global memory on that path.
#include "text_pieces.hpp"

namespace vbt {
namespace {

constexpr uint32_t kDetailBlock = 1024, kDetailWaves = kDetailBlock / 64;  // 16 waves share a tile: 16 sentences in a row per wave
constexpr uint32_t kDetailRound = VBT_DETAIL_ROUND;
constexpr uint32_t kDetailWords = 9;  // per token of a round: output start, surface start, surface length, feature start, tail start, 4 x BCD
static_assert(kScanTile <= kDetailBlock && kScanTile % kDetailWaves == 0 && kScanTile % 64 == 0, "a thread per sentence for the tile's scan");
static_assert(kDetailRound % 64 == 0, "a round is loaded 64 tokens at a time");
// 16 waves x (9 x 64 + 1) words = 36928 bytes, + 2088 of offsets + 72 of labels = 39088: two workgroups (all a CU's wave slots) fit its LDS.
// (A round of 128 would need 75856 bytes.)
static_assert(kDetailWaves * (kDetailWords * kDetailRound + 1) * 4 + (kScanTile + 1 + kScanTile / 64) * 8 + 72 <= 65536,
              "the piece tables, the tile's offsets and the labels within 64 KiB of LDS");

// the label bytes of a tail: five field labels (at 0, 10, 19, 29, 40; 52 bytes), then the lexicon names (at 52, 58, 62)
__constant__ __attribute__((aligned(4))) char kDetailLabels[72] = "\tlex_type=\tleft_id=\tright_id=\tword_cost=\ttotal_cost=SystemUserUnknown";
constexpr uint32_t kLabelBytes = 52;

// what a detail line prints of token k, besides its two strings
struct Fields { uint32_t lex, left, right; int32_t word_cost, total_cost; };

// word_idx and total_cost of the staged record (words 4-5) and the word's 8-byte parameter entry; the index is clamped as
// load_piece clamps its own (memory safety: the device wrote the record itself)
__device__ __forceinline__ Fields load_fields(const BatchArgs& A, const DevWordParams& W, size_t slot, uint32_t k) {
    const uint2 wt = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint32_t*>(A.tok_stage) + 6 * (slot + k) + 4);
    const uint32_t lex = min(wt.x >> 30, 2u), wid = wt.x & 0x3FFFFFFFu;
    const uint32_t nw = lex == 0 ? W.words[0] : lex == 1 ? W.words[1] : W.words[2];
    const uint32_t base = lex == 0 ? W.base[0] : lex == 1 ? W.base[1] : W.base[2];
    const uint2 e = *reinterpret_cast<const uint2*>(W.e + (base + min(wid, nw ? nw - 1u : 0u)));
    return Fields{lex, e.x & 0xFFFFu, e.x >> 16, (int32_t)(int16_t)(e.y & 0xFFFFu), (int32_t)wt.y};
}

__device__ __forceinline__ uint32_t abs_u32(int32_t v) { return v < 0 ? 0u - (uint32_t)v : (uint32_t)v; }  // (INT32_MIN: 2^31)
// decimal digits of v: compares against the powers of ten
__device__ __forceinline__ uint32_t dec_width5(uint32_t v) { return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u); }  // v < 100000
__device__ __forceinline__ uint32_t dec_width10(uint32_t v) {
    return dec_width5(min(v, 99999u)) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}
__device__ __forceinline__ uint32_t lex_name_len(uint32_t lex) { return lex == 0 ? 6u : lex == 1 ? 4u : 7u; }
// bytes of the tail: the labels, the name, the four fields with their signs, '\n'
__device__ __forceinline__ uint32_t tail_len(const Fields& f) {
    return kLabelBytes + lex_name_len(f.lex) + dec_width5(f.left) + dec_width5(f.right) + (f.word_cost < 0) + dec_width5(abs_u32(f.word_cost)) +
           (f.total_cost < 0) + dec_width10(abs_u32(f.total_cost)) + 1u;
}

// packed BCD, digit i (from the right) in nibble i.  v / 10 as a multiply-high: (v * 0xCCCD) >> 19 is exact below 81920
__device__ __forceinline__ uint32_t bcd5(uint32_t v) {
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) { const uint32_t q = (v * 0xCCCDu) >> 19; r |= (v - q * 10u) << (4 * i); v = q; }
    return r;
}
__device__ __forceinline__ uint32_t bcd10(uint32_t v, uint32_t& hi) {  // umulhi(v, ceil(2^35 / 10)) >> 3 is exact for every u32
    uint32_t lo = 0;
    hi = 0;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t q = __umulhi(v, 0xCCCCCCCDu) >> 3, d = v - q * 10u;
        if (i < 8) lo |= d << (4 * i); else hi |= d << (4 * (i - 8));
        v = q;
    }
    return lo;
}

// The four BCD words of a token's table entry:
//   b0 = left_id (20 bits) | lex << 20 | word_cost < 0 << 22 | total_cost < 0 << 23 | digits of left_id << 24
//   b1 = right_id (20)     | digits 8-9 of |total_cost| << 20 | digits of right_id << 28
//   b2 = |word_cost| (20)  | its digits << 20 | digits of |total_cost| << 23
//   b3 = digits 0-7 of |total_cost|
__device__ __forceinline__ uint4 pack_fields(const Fields& f) {
    const uint32_t wc = abs_u32(f.word_cost), tc = abs_u32(f.total_cost);
    uint32_t t_hi;
    const uint32_t t_lo = bcd10(tc, t_hi);
    return uint4{bcd5(f.left) | f.lex << 20 | (uint32_t)(f.word_cost < 0) << 22 | (uint32_t)(f.total_cost < 0) << 23 | dec_width5(f.left) << 24,
                 bcd5(f.right) | t_hi << 20 | dec_width5(f.right) << 28, bcd5(wc) | dec_width5(wc) << 20 | dec_width10(tc) << 23, t_lo};
}

// the fields of one token as a lane that produces bytes of its tail keeps them: decoded once per token, not per byte
struct Tail {
    uint32_t name_at;             // where the lexicon's name starts in the labels
    uint32_t e0, e1, e2, e3, e4;  // cumulative ends of "\tlex_type=name", "\tleft_id=N", "\tright_id=N", "\tword_cost=N", "\ttotal_cost=N"
    uint32_t b0, b1, b2, b3;
};
__device__ __forceinline__ Tail decode_tail(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) {
    Tail t;
    const uint32_t lex = (b0 >> 20) & 3u;
    t.name_at = lex == 0 ? 52u : lex == 1 ? 58u : 62u;
    t.e0 = 10u + lex_name_len(lex);
    t.e1 = t.e0 + 9u + ((b0 >> 24) & 7u);
    t.e2 = t.e1 + 10u + ((b1 >> 28) & 7u);
    t.e3 = t.e2 + 11u + ((b0 >> 22) & 1u) + ((b2 >> 20) & 7u);
    t.e4 = t.e3 + 12u + ((b0 >> 23) & 1u) + ((b2 >> 23) & 15u);
    t.b0 = b0; t.b1 = b1; t.b2 = b2; t.b3 = b3;
    return t;
}
// byte q of the tail: the field by compares, then a label byte (LDS) or a sign or '0' + a nibble
__device__ __forceinline__ uint32_t tail_byte(const Tail& t, uint32_t q, const uint8_t* lab) {
    if (q < t.e0) return lab[min(q < 10u ? q : t.name_at + (q - 10u), 71u)];
    if (q >= t.e4) return (uint32_t)'\n';
    uint32_t s, at, ll, neg = 0, lo, hi = 0;  // the field's start in the tail, its label (where, how long), its sign, its digits
    if (q < t.e1) { s = t.e0; at = 10u; ll = 9u; lo = t.b0 & 0xFFFFFu; }
    else if (q < t.e2) { s = t.e1; at = 19u; ll = 10u; lo = t.b1 & 0xFFFFFu; }
    else if (q < t.e3) { s = t.e2; at = 29u; ll = 11u; neg = (t.b0 >> 22) & 1u; lo = t.b2 & 0xFFFFFu; }
    else { s = t.e3; at = 40u; ll = 12u; neg = (t.b0 >> 23) & 1u; lo = t.b3; hi = (t.b1 >> 20) & 0xFFu; }
    const uint32_t end = q < t.e1 ? t.e1 : q < t.e2 ? t.e2 : q < t.e3 ? t.e3 : t.e4;
    const uint32_t i = q - s;
    if (i < ll) return lab[at + i];
    if (neg && i == ll) return (uint32_t)'-';
    const uint32_t digit = end - 1u - q;  // counted from the right
    return (uint32_t)'0' + ((digit >= 8u ? hi >> (4u * (digit - 8u)) : lo >> (4u * digit)) & 15u);
}

// line_len[s] = per token its surface + '\t' + its feature + its tail, then "EOS\n"
__global__ void __launch_bounds__(kDetailBlock) detail_plan(BatchArgs A, DevFeatures F, DevWordParams W, uint64_t* __restrict__ line_len, uint64_t* __restrict__ tile_bytes) {
    __shared__ unsigned long long tile_total;
    if (A.ctrl[kError] & (uint32_t)kErrFatal) return;
    if (threadIdx.x == 0) tile_total = 0;
    __syncthreads();
    const uint32_t tile0 = blockIdx.x * kScanTile, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t o0 = A.offsets[0];
    unsigned long long mine = 0;
    for (uint32_t j = wave; j < kScanTile; j += kDetailWaves) {
        const uint32_t s = tile0 + j;
        if (s >= A.n) break;
        const uint32_t nt = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.tok_cnt[s]);
        const size_t slot = (size_t)(A.offsets[s] - o0) + (size_t)kSentenceSlack * s;
        uint64_t acc = 0;
        for (uint32_t k = lane; k < nt; k += 64) {
            const Piece p = load_piece(A, F, slot, k);
            acc += (uint64_t)(p.end - p.start) + p.feat_len + 1u + tail_len(load_fields(A, W, slot, k));
        }
        const uint64_t len = wave_sum64(acc) + 4u;
        if (lane == 0) line_len[s] = len;
        mine += len;
    }
    if (lane == 0 && mine) atomicAdd(&tile_total, mine);
    __syncthreads();
    if (threadIdx.x == 0) tile_bytes[blockIdx.x] = tile_total;
}

__global__ void __launch_bounds__(kDetailBlock) detail_render(BatchArgs A, DevFeatures F, DevWordParams W, const uint64_t* __restrict__ line_len,
                                                              const uint64_t* __restrict__ tile_bytes, uint64_t* __restrict__ line_off, uint8_t* __restrict__ out,
                                                              uint64_t out_cap) {
    __shared__ uint64_t wsum[kScanTile / 64];
    __shared__ uint64_t offs[kScanTile + 1];                      // exclusive line offsets of the tile's sentences, relative to the tile
    __shared__ uint32_t t_out[kDetailWaves][kDetailRound + 1];    // per wave, per token of the round: where its output starts in the round's span (+ the end)
    __shared__ uint32_t t_src[kDetailWaves][kDetailRound];        // where its surface starts in the sentence
    __shared__ uint32_t t_len[kDetailWaves][kDetailRound];        // bytes of its surface
    __shared__ uint32_t t_feat[kDetailWaves][kDetailRound];       // where its feature starts in the blob
    __shared__ uint32_t t_tail[kDetailWaves][kDetailRound];       // where its tail starts in the round's span (= where its feature ends)
    __shared__ uint32_t t_bcd[4][kDetailWaves][kDetailRound];     // pack_fields
    __shared__ uint32_t labels[72 / 4];
    if (A.ctrl[kError] & (uint32_t)kErrFatal) return;
    const uint32_t tile0 = blockIdx.x * kScanTile, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t base = tile_bytes[blockIdx.x];
    if (threadIdx.x < 72 / 4) labels[threadIdx.x] = reinterpret_cast<const uint32_t*>(kDetailLabels)[threadIdx.x];
    {   // 64-bit exclusive prefix of the tile's line lengths: the first kScanTile threads, a sentence each
        const uint32_t s = tile0 + threadIdx.x;
        const bool in_tile = threadIdx.x < kScanTile;
        const uint64_t len = in_tile && s < A.n ? line_len[s] : 0ull;
        uint64_t inc = len;
        if (in_tile) {  // (whole waves: kScanTile is a multiple of 64)
            for (uint32_t o = 1; o < 64; o <<= 1) { const uint64_t u = __shfl_up(inc, o); if (lane >= o) inc += u; }
            if (lane == 63) wsum[wave] = inc;
        }
        __syncthreads();
        if (in_tile) {
            uint64_t front = 0;
            for (uint32_t i = 0; i < wave; ++i) front += wsum[i];
            offs[threadIdx.x] = front + inc - len;
            if (s < A.n) line_off[s] = base + front + inc - len;
            if (threadIdx.x == kScanTile - 1) offs[kScanTile] = front + inc;
        }
    }
    __syncthreads();
    const uint64_t o0 = A.offsets[0];
    const uint32_t* __restrict__ blob32 = reinterpret_cast<const uint32_t*>(F.blob);
    const uint8_t* const lab = reinterpret_cast<const uint8_t*>(labels);
    uint32_t* const tab = t_out[wave];
    uint32_t* const src = t_src[wave];
    uint32_t* const slen = t_len[wave];
    uint32_t* const feat = t_feat[wave];
    uint32_t* const tail = t_tail[wave];
    for (uint32_t j = wave; j < kScanTile; j += kDetailWaves) {
        const uint32_t sn = tile0 + j;
        if (sn >= A.n) break;
        const uint32_t nt = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.tok_cnt[sn]);
        const uint64_t line0 = base + offs[j], len = offs[j + 1] - offs[j], line1 = line0 + len;
        if (len >= (1ull << 32) || line1 > out_cap) {  // the line does not fit the output buffer (or 32-bit sizes): flagged, not written
            if (lane == 0) atomicOr(&A.ctrl[kError], (uint32_t)kErrWakatiCap);
            continue;
        }
        const uint64_t sb = A.offsets[sn];
        const uint8_t* __restrict__ txt = A.text + sb;
        const uint32_t nb = (uint32_t)(A.offsets[sn + 1] - sb);
        const uint32_t last_byte = nb ? nb - 1u : 0u;  // (only read when a token has a surface: the sentence is not empty then)
        const size_t slot = (size_t)(sb - o0) + (size_t)kSentenceSlack * sn;
        uint64_t at = line0;  // where the round's output starts
        // (a sentence without tokens: one round without pieces, its span the four bytes of "EOS\n")
        for (uint32_t r0 = 0; r0 < nt || r0 == 0; r0 += kDetailRound) {
            const uint32_t m = min(kDetailRound, nt - r0);
            uint32_t run = 0;  // bytes of the round's pieces
            for (uint32_t c = 0; c < m; c += 64) {
                const uint32_t k = c + lane;
                Piece p{0u, 0u, 0u, 0u};
                Fields f{0u, 0u, 0u, 0, 0};
                if (k < m) { p = load_piece(A, F, slot, r0 + k); f = load_fields(A, W, slot, r0 + k); }
                const uint32_t front = p.end - p.start + 1u + p.feat_len;  // surface, '\t', feature
                uint32_t chunk;
                const uint32_t ex = wave_exscan(k < m ? front + tail_len(f) : 0u, chunk);
                if (k < m) {  // the conversion to decimal: here, once per token
                    const uint4 b = pack_fields(f);
                    tab[k] = run + ex; src[k] = p.start; slen[k] = p.end - p.start; feat[k] = p.feat; tail[k] = run + ex + front;
                    t_bcd[0][wave][k] = b.x; t_bcd[1][wave][k] = b.y; t_bcd[2][wave][k] = b.z; t_bcd[3][wave][k] = b.w;
                }
                run += chunk;
            }
            if (lane == 0) tab[m] = run;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const uint32_t pieces = run;                 // "EOS\n" sits behind the pieces of the line's last round
            const bool ends_line = r0 + m == nt;
            if (ends_line) run += 4u;
            run = (uint32_t)min((uint64_t)run, line1 - at);  // (never beyond the line the plan measured)
            const uint64_t a0 = at & ~3ull;              // the aligned dword the span starts in
            const uint32_t head = (uint32_t)(at - a0);   // bytes of it in front of the span
            const uint32_t nd = (uint32_t)(((uint64_t)head + run + 3u) >> 2);
            for (uint32_t d = lane; d < nd; d += 64) {
                const int64_t rel0 = (int64_t)4 * d - head;  // byte 0 of this lane's dword, relative to the round's output
                const uint32_t first = rel0 < 0 ? 0u : (uint32_t)rel0;
                uint32_t lo = 0, hi = m;  // the token whose output holds byte `first`: the last one that starts at or before it
                while (lo + 1 < hi) { const uint32_t mid = (lo + hi) >> 1; if (tab[mid] <= first) lo = mid; else hi = mid; }
                uint32_t t = lo, word = 0, have = 0;
                uint8_t* const to = out + a0 + (uint64_t)4 * d;
                if (m && rel0 >= 0 && (uint64_t)rel0 + 4u <= run) {
                    // all four bytes inside the feature of token t?  feature bytes are [tab[t] + surface + 1, tail[t])
                    const uint32_t f_begin = tab[t] + slen[t] + 1u, f_end = tail[t];
                    if (first >= f_begin && first + 4u <= f_end) {
                        const uint32_t addr = feat[t] + (first - f_begin);  // absolute in the blob, + 3 inside this feature
                        const uint32_t w0 = blob32[addr >> 2], w1 = blob32[(addr >> 2) + 1];  // (w1: at most the blob's zero slack)
                        *reinterpret_cast<uint32_t*>(to) = __builtin_amdgcn_alignbyte(w1, w0, addr & 3u);
                        continue;
                    }
                }
                uint32_t decoded = ~0u;  // the token `tl` holds the fields of
                Tail tl{};
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int64_t rel = rel0 + b;
                    if (rel < 0 || rel >= (int64_t)run) continue;
                    const uint32_t r = (uint32_t)rel;
                    uint32_t ch;
                    if (r >= pieces) ch = (0x0A534F45u >> (8u * ((r - pieces) & 3u))) & 0xFFu;  // "EOS\n"
                    else {
                        while (r >= tab[t + 1]) ++t;  // (every token has at least its '\t' and its tail: at most one step per dword)
                        const uint32_t in_tok = r - tab[t], sl = slen[t], tail_at = tail[t];
                        if (in_tok < sl) ch = (uint32_t)txt[min(src[t] + in_tok, last_byte)];
                        else if (in_tok == sl) ch = (uint32_t)'\t';
                        else if (r < tail_at) ch = (uint32_t)F.blob[feat[t] + (in_tok - sl - 1u)];
                        else {
                            if (decoded != t) { tl = decode_tail(t_bcd[0][wave][t], t_bcd[1][wave][t], t_bcd[2][wave][t], t_bcd[3][wave][t]); decoded = t; }
                            ch = tail_byte(tl, r - tail_at, lab);
                        }
                    }
                    word |= ch << (8 * b);
                    have |= 1u << b;
                }
                if (have == 0xFu) *reinterpret_cast<uint32_t*>(to) = word;
                else {
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (have >> b & 1u) to[b] = (uint8_t)(word >> (8 * b));
                }
            }
            at += run;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the table is rewritten by the next round)
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// Workspace::render_text_again: the capacity flag of the run is taken back before the lines are rendered into a larger buffer
__global__ void detail_clear_cap_flag(uint32_t* ctrl) { atomicAnd(&ctrl[kError], ~(uint32_t)kErrWakatiCap); }

}  // namespace

namespace kern {

uint32_t detail_round() { return kDetailRound; }
void detail_lines(hipStream_t stream, const BatchArgs& a, const DevFeatures& f, const DevWordParams& w, uint32_t n_tiles, uint64_t* line_len, uint64_t* tile_bytes,
                  uint64_t* line_off, uint8_t* out, uint64_t out_cap, bool count_tokens) {
    if (n_tiles) hipLaunchKernelGGL(vbt::detail_plan, dim3(n_tiles), dim3(kDetailBlock), 0, stream, a, f, w, line_len, tile_bytes);
    text_tile_scan(stream, a, tile_bytes, n_tiles, line_off, count_tokens);
    if (n_tiles) hipLaunchKernelGGL(vbt::detail_render, dim3(n_tiles), dim3(kDetailBlock), 0, stream, a, f, w, line_len, tile_bytes, line_off, out, out_cap);
}
void detail_render_again(hipStream_t stream, const BatchArgs& a, const DevFeatures& f, const DevWordParams& w, uint32_t n_tiles, const uint64_t* line_len,
                         const uint64_t* tile_bytes, uint64_t* line_off, uint8_t* out, uint64_t out_cap) {
    hipLaunchKernelGGL(vbt::detail_clear_cap_flag, dim3(1), dim3(1), 0, stream, a.ctrl);
    if (n_tiles) hipLaunchKernelGGL(vbt::detail_render, dim3(n_tiles), dim3(kDetailBlock), 0, stream, a, f, w, line_len, tile_bytes, line_off, out, out_cap);
}

}  // namespace kern
}  // namespace vbt
