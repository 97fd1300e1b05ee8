// Output in a user-defined format rendered on the device (MeCab's --node-format / --unk-format / --bos-format / --eos-format): per
// sentence the bos bytes, one expansion of the node program per token (the unk program for words of the unknown lexicon), the eos
// bytes.  DESIGN.md section 3.4g; the op program: format.hpp.
//
// format_index (once per compiled format): cuts the feature rows that are already in HBM into the format's field index -- per word
// and wanted CSV field {where its content starts in the blob, how long it is}.  A row of 16 lanes takes a word, a lane one aligned
// dword of the feature per pass (64 bytes per pass: most features are shorter).  The quote state in front of a lane is the parity
// of the quotes in the lanes before it -- a ballot of the lanes' own parities, the row's 16 bits of it, a popcount below the lane
// -- and the ordinal of a comma outside quotes likewise comes from ballots of the lanes' counts; the lane that holds comma number c
// stores the end of field c and the start of field c + 1 if the format wants them (a 256-byte table in LDS says so).  What this
// cannot cut exactly -- a quote that opens anywhere but at the start of a field, or closes anywhere but at its end: a doubled
// quote, bytes behind a closing quote -- puts the word on the exception list with one atomic; the host parses those rows.
//
// format_plan / text_tile_scan / format_render: the scheme of mecab.hip and detail.hip.  A round's LDS table holds per token its
// output start, its surface, its feature, its row of the field index, the widths of its numbers and their digits as packed BCD
// (converted once per token, when the table is filled).  A lane owns one aligned dword of the round's span, finds the token of its
// first byte by binary search and then walks that token's ops, adding up their lengths, until it stands in the op that holds the
// byte; the walk goes on from there for the dword's other bytes, so an op is decoded once per lane and token.  A dword that lies
// inside the content of one field (or of %H) is two aligned loads from the blob and a byte-align; everything else is put together
// byte by byte and leaves as one aligned store, byte stores only at a span's ragged ends.
#include <cstring>

#include "format.hpp"
#include "kernels.hpp"
#include "text_pieces.hpp"  // wave_sum64

namespace vbt {
namespace {

constexpr uint32_t kFormatBlock = 1024, kFormatWaves = kFormatBlock / 64;  // 16 waves share a tile: 16 sentences in a row per wave
constexpr uint32_t kFormatRound = VBT_FORMAT_ROUND;
// per token of a round: output start, surface start, surface length, feature start, feature length, index row, widths, 8 x BCD
constexpr uint32_t kFormatWords = 15;
static_assert(kScanTile <= kFormatBlock && kScanTile % kFormatWaves == 0 && kScanTile % 64 == 0, "a thread per sentence for the tile's scan");
static_assert(kFormatRound % 64 == 0, "a round is loaded 64 tokens at a time");
// 16 waves x (15 x 64 + 1) words = 61504 bytes, + 2088 of offsets + 1320 of program = 64912: two workgroups (all a CU's wave slots)
// fit its 160 KiB of LDS, and one stays below the 64 KiB a workgroup may declare.  (A round of 128 would need 126 KiB.)
static_assert(kFormatWaves * (kFormatWords * kFormatRound + 1) * 4 + (kScanTile + 1 + kScanTile / 64) * 8 + sizeof(FmtProgram) <= 65536,
              "the token tables, the tile's offsets and the program within 64 KiB of LDS");
static_assert(2 * (kFormatWaves * (kFormatWords * kFormatRound + 1) * 4 + (kScanTile + 1 + kScanTile / 64) * 8 + sizeof(FmtProgram)) <= 160 * 1024,
              "two workgroups in a CU's LDS");

// ---------------------------------------------------------------- the field index

constexpr uint32_t kIndexBlock = 256, kIndexLanes = 16, kIndexRows = kIndexBlock / kIndexLanes;
static_assert(kFmtMaxSlots <= kIndexLanes, "a lane of the row per slot");

// exc[0] = words on the exception list, exc[1 ..] = their rows (room for every row)
__global__ void __launch_bounds__(kIndexBlock) format_index(DevFeatures F, uint32_t rows, FmtProgram prog, uint2* __restrict__ index,
                                                            uint32_t* __restrict__ exc) {
    __shared__ uint8_t slot_of[256];  // CSV field -> slot, 0xFF: the format does not print it
    __shared__ uint32_t f_start[kIndexRows][kIndexLanes], f_end[kIndexRows][kIndexLanes];
    const uint32_t slots = min(prog.slots, kFmtMaxSlots);
    const uint32_t g = threadIdx.x / kIndexLanes, li = threadIdx.x % kIndexLanes, row = blockIdx.x * kIndexRows + g;
    const uint32_t row_shift = threadIdx.x & 48u;  // where this row's 16 bits start in a ballot of its wave
    slot_of[threadIdx.x] = 0xFF;
    __syncthreads();
    if (threadIdx.x < slots) slot_of[prog.field[threadIdx.x]] = (uint8_t)threadIdx.x;
    const bool live = row < rows;
    const uint32_t f0 = live ? F.off[row] : 0u, f1 = max(live ? F.off[row + 1] : 0u, f0);
    f_start[g][li] = li < slots && prog.field[li] == 0 ? f0 : 0xFFFFFFFFu;  // field 0 starts with the row
    f_end[g][li] = 0xFFFFFFFFu;
    __syncthreads();
    const uint32_t* __restrict__ blob32 = reinterpret_cast<const uint32_t*>(F.blob);
    uint32_t in_quote = 0, commas = 0, bad = 0;  // of the row, in front of this pass
    for (uint32_t a = f0 & ~3u;; a += 4 * kIndexLanes) {
        if (__ballot(a < f1) == 0) break;  // (wave-uniform: the ballots below want every row of the wave)
        const uint32_t p0 = a + 4 * li;
        const bool mine = p0 < f1;
        const uint32_t w = mine ? blob32[p0 >> 2] : 0u;  // (at most 3 bytes behind the feature: the next one's, or the blob's zero slack)
        // the bytes around the dword; the row's ends count as commas
        const uint32_t before = mine && p0 > f0 ? F.blob[p0 - 1] : (uint32_t)',', behind = mine && p0 + 4 < f1 ? F.blob[p0 + 4] : (uint32_t)',';
        uint32_t quotes = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (p0 + j >= f0 && p0 + j < f1 && ((w >> (8 * j)) & 0xFFu) == '"') quotes ^= 1u;
        const uint32_t qrow = (uint32_t)(__ballot(quotes != 0) >> row_shift) & 0xFFFFu;
        uint32_t q = in_quote ^ (__popc(qrow & ((1u << li) - 1u)) & 1u);
        in_quote ^= __popc(qrow) & 1u;
        uint32_t cmask = 0;  // the dword's commas outside quotes
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t p = p0 + j, c = (w >> (8 * j)) & 0xFFu;
            if (p < f0 || p >= f1) continue;
            if (c == '"') {
                // an opening quote stands at the start of a field, a closing one at its end
                const uint32_t prev = p == f0 ? (uint32_t)',' : j ? (w >> (8 * (j ? j - 1 : 0))) & 0xFFu : before;
                const uint32_t next = p + 1 == f1 ? (uint32_t)',' : j < 3 ? (w >> (8 * (j < 3 ? j + 1 : 3))) & 0xFFu : behind;
                if ((q ? next : prev) != ',') bad = 1;
                q ^= 1u;
            } else if (c == ',' && !q) cmask |= 1u << j;
        }
        const uint32_t nc = __popc(cmask);  // 0 .. 4: its prefix over the row from three ballots
        const uint32_t below = (1u << li) - 1u;
        const uint32_t b0 = (uint32_t)(__ballot(nc & 1u) >> row_shift) & 0xFFFFu, b1 = (uint32_t)(__ballot(nc & 2u) >> row_shift) & 0xFFFFu,
                       b2 = (uint32_t)(__ballot(nc & 4u) >> row_shift) & 0xFFFFu;
        uint32_t ord = commas + __popc(b0 & below) + 2u * __popc(b1 & below) + 4u * __popc(b2 & below);
        commas += __popc(b0) + 2u * __popc(b1) + 4u * __popc(b2);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            if (!(cmask >> j & 1u)) continue;
            if (ord < 256u) {  // comma number `ord` ends field ord and starts field ord + 1
                const uint32_t se = slot_of[ord], ss = ord < 255u ? slot_of[ord + 1] : 0xFFu;
                if (se < kIndexLanes) f_end[g][se] = p0 + j;
                if (ss < kIndexLanes) f_start[g][ss] = p0 + j + 1u;
            }
            ++ord;
        }
    }
    __syncthreads();
    if (in_quote) bad = 1;  // (a quote that never closes)
    const uint32_t bad_row = (uint32_t)(__ballot(bad != 0) >> row_shift) & 0xFFFFu;
    if (!live) return;
    if (li < slots) {
        const uint32_t st = f_start[g][li];
        uint2 e{0u, kFmtAbsent};
        if (st != 0xFFFFFFFFu) {
            const uint32_t en = f_end[g][li] == 0xFFFFFFFFu ? f1 : f_end[g][li];  // (the last field ends with the row)
            e.x = st;
            e.y = en - st;
            if (e.y >= 2u && F.blob[st] == '"') { e.x += 1u; e.y -= 2u; }  // a quoted field: what is between its quotes
            e.y &= kFmtLenMask;
            if (e.y == 1u && F.blob[e.x] == '*') e.y |= kFmtStar;
        }
        index[(size_t)row * slots + li] = e;
    }
    if (li == 0 && bad_row) exc[1u + atomicAdd(&exc[0], 1u)] = row;
}

// ---------------------------------------------------------------- a token and its ops

// what the ops of token k read: its surface, its lexicon, its row of DevFeatures::off (= of the field index), its total cost
struct Tok { uint32_t start, end, lex, wid, row; int32_t total; };

// words 2-5 of record k of the staging region that starts at `slot`; the word index is clamped as load_piece clamps it
__device__ __forceinline__ Tok load_tok(const BatchArgs& A, const DevFeatures& F, size_t slot, uint32_t k) {
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(A.tok_stage) + 6 * (slot + k);
    const uint2 se = *reinterpret_cast<const uint2*>(rec + 2), wt = *reinterpret_cast<const uint2*>(rec + 4);
    const uint32_t lex = min(wt.x >> 30, 2u), wid = wt.x & 0x3FFFFFFFu;
    const uint32_t nw = lex == 0 ? F.words[0] : lex == 1 ? F.words[1] : F.words[2];
    const uint32_t base = lex == 0 ? F.base[0] : lex == 1 ? F.base[1] : F.base[2];
    return Tok{se.x, max(se.y, se.x), lex, wid, base + min(wid, nw ? nw - 1u : 0u), (int32_t)wt.y};
}

// (the small decimal helpers of detail.hip, which is not to change: kept the same here)
__device__ __forceinline__ uint32_t abs_u32(int32_t v) { return v < 0 ? 0u - (uint32_t)v : (uint32_t)v; }  // (INT32_MIN: 2^31)
__device__ __forceinline__ uint32_t dec_width5(uint32_t v) { return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u); }  // v < 100000
__device__ __forceinline__ uint32_t dec_width10(uint32_t v) {
    return dec_width5(min(v, 99999u)) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}
__device__ __forceinline__ uint32_t bcd5(uint32_t v) {  // (v * 0xCCCD) >> 19 = v / 10 below 81920
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) { const uint32_t q = (v * 0xCCCDu) >> 19; r |= (v - q * 10u) << (4 * i); v = q; }
    return r;
}
__device__ __forceinline__ uint32_t bcd10(uint32_t v, uint32_t& hi) {  // umulhi(v, ceil(2^35 / 10)) >> 3 = v / 10 for every u32
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

// the numbers a token's ops may print
struct Nums { uint32_t left, right; int32_t word_cost, total; uint32_t start, end; };
__device__ __forceinline__ Nums load_nums(const Tok& t, const DevWordParams& W, uint32_t uses) {
    Nums n{0u, 0u, 0, t.total, t.start, t.end};
    if (uses & kFmtUsesParams) {  // the DICTIONARY's ids (DevWordParams), never the device ids of an image's entries
        const uint32_t nw = t.lex == 0 ? W.words[0] : t.lex == 1 ? W.words[1] : W.words[2];
        const uint32_t base = t.lex == 0 ? W.base[0] : t.lex == 1 ? W.base[1] : W.base[2];
        const uint2 e = *reinterpret_cast<const uint2*>(W.e + (base + min(t.wid, nw ? nw - 1u : 0u)));
        n.left = e.x & 0xFFFFu; n.right = e.x >> 16; n.word_cost = (int32_t)(int16_t)(e.y & 0xFFFFu);
    }
    return n;
}
// Nibble kind - kFmtLeft = bytes the number of that kind prints, its sign included (compares against the powers of ten);
// bits 28-29 the lexicon, bit 30 word_cost < 0, bit 31 total_cost < 0.
__device__ __forceinline__ uint32_t pack_widths(uint32_t lex, const Nums& n, uint32_t uses) {
    uint32_t w = lex << 28;
    if (uses & kFmtUsesNumbers)
        w |= dec_width5(n.left) | dec_width5(n.right) << 4 | ((n.word_cost < 0) + dec_width5(abs_u32(n.word_cost))) << 8 |
             ((n.total < 0) + dec_width10(abs_u32(n.total))) << 12 | dec_width10(n.start) << 16 | dec_width10(n.end) << 20 | dec_width10(n.end - n.start) << 24 |
             (uint32_t)(n.word_cost < 0) << 30 | (uint32_t)(n.total < 0) << 31;
    return w;
}

// One op of a token: how many bytes it prints, and for a field what they are.  `printed`: a field of the %F list this op belongs to
// has been printed.  sepn: 1 when the op's separator byte goes in front of the content.
struct FieldSrc { uint32_t off, len, sepn, side; };
__device__ __forceinline__ uint32_t op_len(uint32_t op, uint32_t slen, uint32_t flen, uint32_t widths, const uint2* __restrict__ idx_row, bool& printed, FieldSrc& fs) {
    const uint32_t kind = op & 0xFFu;
    if (kind == kFmtLit) return op >> 20;
    if (kind == kFmtSurface) return slen;
    if (kind == kFmtFeature) return flen;
    if (kind == kFmtIsUnk) return 1u;
    if (kind != kFmtField) return (widths >> (4u * min(kind - kFmtLeft, 6u))) & 15u;
    const uint32_t flags = op >> 20;
    const uint2 e = idx_row[(op >> 8) & 15u];
    const bool present = e.y != kFmtAbsent;
    if (flags & kFmtFirst) printed = false;
    bool show = present;
    uint32_t sepn = flags & kFmtSep ? 1u : 0u;
    if (flags & kFmtSkip) {
        show = present && !(e.y & kFmtStar);
        sepn = show && printed ? 1u : 0u;
        printed = printed || show;
    }
    fs = FieldSrc{e.x, show ? e.y & kFmtLenMask : 0u, sepn, show ? e.y & kFmtSide : 0u};
    return fs.sepn + fs.len;
}

// bytes the program prints for one token
__device__ __forceinline__ uint32_t token_len(const uint32_t* ops, uint32_t n_ops, uint32_t slen, uint32_t flen, uint32_t widths, const uint2* __restrict__ idx_row) {
    uint32_t len = 0;
    bool printed = false;
    FieldSrc fs;
    for (uint32_t i = 0; i < n_ops; ++i) len += op_len(ops[i], slen, flen, widths, idx_row, printed, fs);
    return len;
}

// the program, from the kernel arguments into LDS: once per workgroup (the caller synchronises)
__device__ __forceinline__ void load_program(FmtProgram& prog, const FmtProgram& from) {
    for (uint32_t i = threadIdx.x; i < sizeof(FmtProgram) / 4; i += blockDim.x) reinterpret_cast<uint32_t*>(&prog)[i] = reinterpret_cast<const uint32_t*>(&from)[i];
}

// ---------------------------------------------------------------- plan

// line_len[s] = bos + per token the bytes of its program + eos
__global__ void __launch_bounds__(kFormatBlock) format_plan(BatchArgs A, DevFeatures F, DevWordParams W, DevFormat D, uint64_t* __restrict__ line_len,
                                                            uint64_t* __restrict__ tile_bytes) {
    __shared__ unsigned long long tile_total;
    __shared__ FmtProgram prog;
    if (A.ctrl[kError] & (uint32_t)kErrFatal) return;
    if (threadIdx.x == 0) tile_total = 0;
    load_program(prog, D.prog);
    __syncthreads();
    const uint32_t tile0 = blockIdx.x * kScanTile, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t uses = prog.uses, slots = min(prog.slots, kFmtMaxSlots);
    const uint32_t n_ops[2] = {min(prog.n_ops[0], kFmtMaxOps), min(prog.n_ops[1], kFmtMaxOps)};
    const uint64_t o0 = A.offsets[0];
    unsigned long long mine = 0;
    for (uint32_t j = wave; j < kScanTile; j += kFormatWaves) {
        const uint32_t s = tile0 + j;
        if (s >= A.n) break;
        const uint32_t nt = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.tok_cnt[s]);
        const size_t slot = (size_t)(A.offsets[s] - o0) + (size_t)kSentenceSlack * s;
        uint64_t acc = 0;
        for (uint32_t k = lane; k < nt; k += 64) {
            const Tok t = load_tok(A, F, slot, k);
            const uint32_t flen = uses & kFmtUsesFeature ? F.off[t.row + 1] - F.off[t.row] : 0u;
            const uint32_t which = t.lex == 2u;
            acc += token_len(prog.ops[which], which ? n_ops[1] : n_ops[0], t.end - t.start, flen, pack_widths(t.lex, load_nums(t, W, uses), uses),
                             D.index + (size_t)t.row * slots);
        }
        const uint64_t len = wave_sum64(acc) + prog.bos_len + prog.eos_len;
        if (lane == 0) line_len[s] = len;
        mine += len;
    }
    if (lane == 0 && mine) atomicAdd(&tile_total, mine);
    __syncthreads();
    if (threadIdx.x == 0) tile_bytes[blockIdx.x] = tile_total;
}

// ---------------------------------------------------------------- render

// Where a lane stands in the program of one token: ops[0 .. i) have been added up, the last of them prints the token's bytes [s, e).
struct Walk {
    uint32_t i, s, e, kind, lit;
    bool printed;
    FieldSrc fs;
};

__global__ void __launch_bounds__(kFormatBlock) format_render(BatchArgs A, DevFeatures F, DevWordParams W, DevFormat D, const uint64_t* __restrict__ line_len,
                                                              const uint64_t* __restrict__ tile_bytes, uint64_t* __restrict__ line_off, uint8_t* __restrict__ out,
                                                              uint64_t out_cap) {
    __shared__ uint64_t wsum[kScanTile / 64];
    __shared__ uint64_t offs[kScanTile + 1];                      // exclusive line offsets of the tile's sentences, relative to the tile
    __shared__ uint32_t t_out[kFormatWaves][kFormatRound + 1];    // per wave, per token of the round: where its output starts in the round's span (+ the end)
    __shared__ uint32_t t_src[kFormatWaves][kFormatRound];        // where its surface starts in the sentence
    __shared__ uint32_t t_len[kFormatWaves][kFormatRound];        // bytes of its surface
    __shared__ uint32_t t_feat[kFormatWaves][kFormatRound];       // where its feature starts in the blob
    __shared__ uint32_t t_flen[kFormatWaves][kFormatRound];       // bytes of its feature
    __shared__ uint32_t t_row[kFormatWaves][kFormatRound];        // its row of the field index
    __shared__ uint32_t t_wid[kFormatWaves][kFormatRound];        // pack_widths
    // the digits, packed BCD (digit i from the right in nibble i): [0] total_cost 0-7, [1] start 0-7, [2] end 0-7, [3] length 0-7,
    // [4] left_id | digits 8-9 of total_cost << 20, [5] right_id, [6] |word_cost|, [7] digits 8-9 of start | of end << 8 | of length << 16
    __shared__ uint32_t t_bcd[8][kFormatWaves][kFormatRound];
    __shared__ FmtProgram prog;
    if (A.ctrl[kError] & (uint32_t)kErrFatal) return;
    const uint32_t tile0 = blockIdx.x * kScanTile, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t base = tile_bytes[blockIdx.x];
    load_program(prog, D.prog);
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
    const uint32_t uses = prog.uses, slots = min(prog.slots, kFmtMaxSlots);
    const uint32_t n_ops0 = min(prog.n_ops[0], kFmtMaxOps), n_ops1 = min(prog.n_ops[1], kFmtMaxOps);
    const uint32_t bos_len = min(prog.bos_len, kFmtMaxLit), eos_len = min(prog.eos_len, kFmtMaxLit);
    const uint64_t o0 = A.offsets[0];
    const uint32_t* __restrict__ blob32 = reinterpret_cast<const uint32_t*>(F.blob);
    const uint32_t* __restrict__ side32 = reinterpret_cast<const uint32_t*>(D.side);
    uint32_t* const tab = t_out[wave];
    for (uint32_t j = wave; j < kScanTile; j += kFormatWaves) {
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
        // (a sentence without tokens: one round without tokens, its span bos and eos)
        for (uint32_t r0 = 0; r0 < nt || r0 == 0; r0 += kFormatRound) {
            const uint32_t m = min(kFormatRound, nt - r0);
            const uint32_t head_len = r0 == 0 ? bos_len : 0u;  // bos stands in front of the tokens of the line's first round
            uint32_t run = head_len;
            for (uint32_t c = 0; c < m; c += 64) {
                const uint32_t k = c + lane;
                Tok t{0u, 0u, 0u, 0u, 0u, 0};
                uint32_t tl = 0, widths = 0, feat = 0, flen = 0;
                Nums nm{0u, 0u, 0, 0, 0u, 0u};
                if (k < m) {
                    t = load_tok(A, F, slot, r0 + k);
                    if (uses & kFmtUsesFeature) { feat = F.off[t.row]; flen = F.off[t.row + 1] - feat; }
                    nm = load_nums(t, W, uses);
                    widths = pack_widths(t.lex, nm, uses);
                    const bool unk = t.lex == 2u;
                    tl = token_len(prog.ops[unk], unk ? n_ops1 : n_ops0, t.end - t.start, flen, widths, D.index + (size_t)t.row * slots);
                }
                uint32_t chunk;
                const uint32_t ex = wave_exscan(tl, chunk);
                if (k < m) {
                    tab[k] = run + ex; t_src[wave][k] = t.start; t_len[wave][k] = t.end - t.start; t_feat[wave][k] = feat; t_flen[wave][k] = flen;
                    t_row[wave][k] = t.row; t_wid[wave][k] = widths;
                    if (uses & kFmtUsesNumbers) {  // the conversion to decimal: here, once per token
                        uint32_t h_tc, h_s, h_e, h_l;
                        t_bcd[0][wave][k] = bcd10(abs_u32(nm.total), h_tc);
                        t_bcd[1][wave][k] = bcd10(nm.start, h_s);
                        t_bcd[2][wave][k] = bcd10(nm.end, h_e);
                        t_bcd[3][wave][k] = bcd10(nm.end - nm.start, h_l);
                        t_bcd[4][wave][k] = bcd5(nm.left) | h_tc << 20;
                        t_bcd[5][wave][k] = bcd5(nm.right);
                        t_bcd[6][wave][k] = bcd5(abs_u32(nm.word_cost));
                        t_bcd[7][wave][k] = h_s | h_e << 8 | h_l << 16;
                    }
                }
                run += chunk;
            }
            if (lane == 0) tab[m] = run;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const uint32_t pieces = run;  // eos stands behind the tokens of the line's last round
            if (r0 + m == nt) run += eos_len;
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
                Walk wk{0u, 0u, 0u, 0u, 0u, false, FieldSrc{0u, 0u, 0u, 0u}};
                uint32_t walked = ~0u;  // the token `wk` walks
                bool stored = false;
#pragma unroll
                for (int b = 0; b < 4 && !stored; ++b) {
                    const int64_t rel = rel0 + b;
                    if (rel < 0 || rel >= (int64_t)run) continue;
                    const uint32_t r = (uint32_t)rel;
                    uint32_t ch;
                    if (r < head_len) ch = prog.bos[r & (kFmtMaxLit - 1u)];
                    else if (r >= pieces) ch = prog.eos[(r - pieces) & (kFmtMaxLit - 1u)];
                    else {
                        while (r >= tab[t + 1]) ++t;  // (r < pieces = tab[m]: ends at m - 1 at the latest; tokens may print nothing)
                        if (walked != t) { wk = Walk{0u, 0u, 0u, 0u, 0u, false, FieldSrc{0u, 0u, 0u, 0u}}; walked = t; }
                        const uint32_t q = r - tab[t], widths = t_wid[wave][t];
                        const bool unk = ((widths >> 28) & 3u) == 2u;
                        const uint32_t* ops = prog.ops[unk];
                        const uint32_t n_ops = unk ? n_ops1 : n_ops0;
                        while (q >= wk.e && wk.i < n_ops) {  // on to the op that prints byte q of the token
                            const uint32_t op = ops[wk.i++];
                            wk.s = wk.e;
                            wk.kind = op & 0xFFu;
                            wk.lit = (op >> 8) & 0xFFFu;
                            wk.e += op_len(op, t_len[wave][t], t_flen[wave][t], widths, D.index + (size_t)t_row[wave][t] * slots, wk.printed, wk.fs);
                            if (wk.kind == kFmtFeature) wk.fs = FieldSrc{t_feat[wave][t], t_flen[wave][t], 0u, 0u};
                        }
                        const uint32_t i = q - wk.s;  // byte i of the op
                        if (q >= wk.e) ch = (uint32_t)'?';  // (the ops add up to the token's length: not reached)
                        else if (wk.kind == kFmtFeature || wk.kind == kFmtField) {
                            if (i < wk.fs.sepn) ch = (wk.lit >> 4) & 0xFFu;
                            else {
                                const uint32_t addr = wk.fs.off + (i - wk.fs.sepn);
                                if (b == 0 && rel0 >= 0 && (uint64_t)rel0 + 4u <= run && i - wk.fs.sepn + 4u <= wk.fs.len) {
                                    // all four bytes inside this content: two aligned loads and a byte-align
                                    const uint32_t* src = wk.fs.side ? side32 : blob32;
                                    const uint32_t w0 = src[addr >> 2], w1 = src[(addr >> 2) + 1];  // (w1: at most the blob's zero slack)
                                    *reinterpret_cast<uint32_t*>(to) = __builtin_amdgcn_alignbyte(w1, w0, addr & 3u);
                                    stored = true;
                                    continue;
                                }
                                ch = (uint32_t)(wk.fs.side ? D.side : F.blob)[addr];
                            }
                        } else if (wk.kind == kFmtLit) ch = prog.lit[unk][(wk.lit + i) & (kFmtMaxLit - 1u)];
                        else if (wk.kind == kFmtSurface) ch = (uint32_t)txt[min(t_src[wave][t] + i, last_byte)];
                        else if (wk.kind == kFmtIsUnk) ch = (uint32_t)'0' + (uint32_t)unk;
                        else {  // a number: its sign, or '0' + a nibble
                            const uint32_t neg = wk.kind == kFmtWordCost ? (widths >> 30) & 1u : wk.kind == kFmtTotalCost ? widths >> 31 : 0u;
                            if (neg && i == 0) ch = (uint32_t)'-';
                            else {
                                const uint32_t digit = wk.e - 1u - q;  // counted from the right
                                const uint32_t n = min(wk.kind - kFmtLeft, 6u);  // left, right, word cost, total cost, start, end, length
                                const uint32_t lo_word = n == 0 ? 4u : n == 1 ? 5u : n == 2 ? 6u : n - 3u;
                                const uint32_t lo_digits = t_bcd[lo_word][wave][t] & (n < 3 ? 0xFFFFFu : 0xFFFFFFFFu);
                                const uint32_t hi_digits = n < 3 ? 0u : n == 3 ? t_bcd[4][wave][t] >> 20 : (t_bcd[7][wave][t] >> (8u * (n - 4u))) & 0xFFu;
                                ch = (uint32_t)'0' + ((digit >= 8u ? hi_digits >> (4u * (digit - 8u)) : lo_digits >> (4u * digit)) & 15u);
                            }
                        }
                    }
                    word |= ch << (8 * b);
                    have |= 1u << b;
                }
                if (stored) continue;
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
__global__ void format_clear_cap_flag(uint32_t* ctrl) { atomicAnd(&ctrl[kError], ~(uint32_t)kErrWakatiCap); }
__global__ void format_clear_words(uint32_t* p, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0;
}
// the exception rows' entries as the host made them: thread i * slots + s patches slot s of row exc[1 + i]
__global__ void format_patch(uint2* __restrict__ index, const uint32_t* __restrict__ exc, const uint2* __restrict__ patch, uint32_t n_exc, uint32_t slots, uint32_t rows) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)n_exc * slots) return;
    const uint32_t row = exc[1u + (uint32_t)(i / slots)];
    if (row < rows) index[(size_t)row * slots + (uint32_t)(i % slots)] = patch[i];
}

}  // namespace

namespace kern {

void format_index(hipStream_t stream, const DevFeatures& f, uint32_t rows, const FmtProgram& prog, uint2* index, uint32_t* exc) {
    hipLaunchKernelGGL(vbt::format_clear_words, dim3(1), dim3(64), 0, stream, exc, 1u);
    if (rows) hipLaunchKernelGGL(vbt::format_index, dim3((rows + kIndexRows - 1) / kIndexRows), dim3(kIndexBlock), 0, stream, f, rows, prog, index, exc);
}
void format_patch(hipStream_t stream, uint2* index, const uint32_t* exc, const uint2* patch, uint32_t n_exc, uint32_t slots, uint32_t rows) {
    const uint64_t n = (uint64_t)n_exc * slots;
    if (n) hipLaunchKernelGGL(vbt::format_patch, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, index, exc, patch, n_exc, slots, rows);
}
void format_lines(hipStream_t stream, const BatchArgs& a, const DevFeatures& f, const DevWordParams& w, const DevFormat& d, uint32_t n_tiles, uint64_t* line_len,
                  uint64_t* tile_bytes, uint64_t* line_off, uint8_t* out, uint64_t out_cap, bool count_tokens) {
    if (n_tiles) hipLaunchKernelGGL(vbt::format_plan, dim3(n_tiles), dim3(kFormatBlock), 0, stream, a, f, w, d, line_len, tile_bytes);
    text_tile_scan(stream, a, tile_bytes, n_tiles, line_off, count_tokens);
    if (n_tiles) hipLaunchKernelGGL(vbt::format_render, dim3(n_tiles), dim3(kFormatBlock), 0, stream, a, f, w, d, line_len, tile_bytes, line_off, out, out_cap);
}
void format_render_again(hipStream_t stream, const BatchArgs& a, const DevFeatures& f, const DevWordParams& w, const DevFormat& d, uint32_t n_tiles,
                         const uint64_t* line_len, const uint64_t* tile_bytes, uint64_t* line_off, uint8_t* out, uint64_t out_cap) {
    hipLaunchKernelGGL(vbt::format_clear_cap_flag, dim3(1), dim3(1), 0, stream, a.ctrl);
    if (n_tiles) hipLaunchKernelGGL(vbt::format_render, dim3(n_tiles), dim3(kFormatBlock), 0, stream, a, f, w, d, line_len, tile_bytes, line_off, out, out_cap);
}

}  // namespace kern

// ---------------------------------------------------------------- the compiled format's device side

Format::~Format() {
    for (void* p : allocs_)
        if (p) { (void)hipSetDevice(device_); (void)hipFree(p); }
}

const DevFormat& Format::device() const {
    std::call_once(once_, [&] {  // (a throw leaves the flag unset: the next caller tries again)
        const DevFeatures& F = tok.feature_table();
        const FlatFeatures* flat = tok.flat_features();
        const uint32_t rows = F.base[2] + F.words[2] + 1u;  // every entry of off[] that has a successor
        const uint32_t slots = prog.slots;
        HIP_CHECK(hipSetDevice(device_));
        void *d_index = nullptr, *d_side = nullptr, *d_exc = nullptr, *d_patch = nullptr;
        try {
            HIP_CHECK(hipMalloc(&d_index, std::max<size_t>((size_t)rows * slots, 1) * sizeof(uint2)));
            std::vector<uint8_t> side;
            if (slots) {
                uint32_t n_exc = 0;
                HIP_CHECK(hipMalloc(&d_exc, ((size_t)rows + 1) * 4));
                kern::format_index(nullptr, F, rows, prog, static_cast<uint2*>(d_index), static_cast<uint32_t*>(d_exc));
                HIP_CHECK(hipGetLastError());
                HIP_CHECK(hipMemcpy(&n_exc, d_exc, 4, hipMemcpyDeviceToHost));
                if (n_exc > rows) throw Error(VBT_ERR_DEVICE, "format_index: the exception list is longer than the table");
                std::vector<uint32_t> exc(n_exc);
                if (n_exc) HIP_CHECK(hipMemcpy(exc.data(), static_cast<uint32_t*>(d_exc) + 1, (size_t)n_exc * 4, hipMemcpyDeviceToHost));
                // the rows the kernel could not cut: parse_csv_row's fields go into the side blob, and the rows' new entries -- in the
                // list's order, ONE upload however many there are -- are put in place by format_patch
                std::vector<uint2> patch((size_t)n_exc * slots, uint2{0u, kFmtAbsent});
                for (uint32_t i = 0; i < n_exc; ++i) {
                    const uint32_t row = exc[i];
                    int l = 2;
                    while (l > 0 && row < F.base[l]) --l;
                    const uint32_t id = row - F.base[l];
                    if (row >= rows || id >= F.words[l]) continue;  // (a terminator row: no word)
                    const FlatFeatures& ff = flat[l];
                    const std::vector<std::string> fields = parse_csv_row(std::string_view(ff.blob.data() + ff.off[id], ff.off[id + 1] - ff.off[id]));
                    for (uint32_t s = 0; s < slots; ++s) {
                        if (prog.field[s] >= fields.size()) continue;
                        const std::string& c = fields[prog.field[s]];
                        if (side.size() + c.size() >= kFmtSide) throw Error(VBT_ERR_UNSUPPORTED, "format: 1 GiB of re-parsed field text");
                        patch[(size_t)i * slots + s] = uint2{(uint32_t)side.size(), (uint32_t)c.size() | kFmtSide | (c == "*" ? kFmtStar : 0u)};
                        side.insert(side.end(), c.begin(), c.end());
                    }
                }
                if (n_exc) {
                    HIP_CHECK(hipMalloc(&d_patch, patch.size() * sizeof(uint2)));
                    HIP_CHECK(hipMemcpy(d_patch, patch.data(), patch.size() * sizeof(uint2), hipMemcpyHostToDevice));
                    kern::format_patch(nullptr, static_cast<uint2*>(d_index), static_cast<const uint32_t*>(d_exc), static_cast<const uint2*>(d_patch), n_exc, slots, rows);
                    HIP_CHECK(hipGetLastError());
                }
            }
            const size_t side_alloc = (side.size() + 8 + 3) & ~(size_t)3;  // the zero slack of the feature blob
            side.resize(side_alloc, 0);
            HIP_CHECK(hipMalloc(&d_side, side_alloc));
            HIP_CHECK(hipMemcpy(d_side, side.data(), side_alloc, hipMemcpyHostToDevice));
            HIP_CHECK(hipDeviceSynchronize());  // (everything has landed before a kernel of any stream reads the tables)
            for (void** p : {&d_exc, &d_patch})
                if (*p) { (void)hipFree(*p); *p = nullptr; }
        } catch (...) {
            for (void* p : {d_index, d_side, d_exc, d_patch})
                if (p) (void)hipFree(p);
            throw;
        }
        allocs_[0] = d_index; allocs_[1] = d_side;
        dev_.index = static_cast<const uint2*>(d_index);
        dev_.side = static_cast<const uint8_t*>(d_side);
    });
    return dev_;
}

}  // namespace vbt
