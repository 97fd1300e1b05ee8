// What the two renderers that read the feature table share (mecab.hip, detail.hip): a token's two sources -- its surface in the
// sentence, its feature in the blob -- from the staged record, and a 64-bit sum over a wave.
#pragma once
#include "device_common.hpp"

namespace vbt {
namespace {

struct Piece { uint32_t start, end, feat, feat_len; };  // of one token: its surface in the sentence, its feature in the blob

// {start_byte, end_byte, word_idx} of record k of the staging region that starts at `slot` (words 2-4 of the 24-byte record) and the
// two offsets of its feature.  A word index outside the table -- the device wrote the record itself, so this is memory safety, not
// an input that is served -- is clamped to the table: a lexicon tag above 2 to the unknown lexicon, an id to the lexicon's last.
// (off[] ends with one entry more than the lexicons have, so that an EMPTY lexicon's entry 0 and 1 are inside it as well.)
__device__ __forceinline__ Piece load_piece(const BatchArgs& A, const DevFeatures& F, size_t slot, uint32_t k) {
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(A.tok_stage) + 6 * (slot + k);
    const uint2 se = *reinterpret_cast<const uint2*>(rec + 2);
    const uint32_t widx = rec[4];
    const uint32_t lex = min(widx >> 30, 2u), wid = widx & 0x3FFFFFFFu;
    const uint32_t nw = lex == 0 ? F.words[0] : lex == 1 ? F.words[1] : F.words[2];
    const uint32_t base = lex == 0 ? F.base[0] : lex == 1 ? F.base[1] : F.base[2];
    const uint32_t i = base + min(wid, nw ? nw - 1u : 0u);
    const uint32_t f0 = F.off[i], f1 = F.off[i + 1];
    return Piece{se.x, se.y, f0, f1 - f0};
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {  // in three 24-bit limbs (64 of them add up inside 32 bits)
    const uint64_t a = wave_sum((uint32_t)v & 0xFFFFFFu), b = wave_sum((uint32_t)(v >> 24) & 0xFFFFFFu), c = wave_sum((uint32_t)(v >> 48));
    return a + (b << 24) + (c << 48);
}

}  // namespace
}  // namespace vbt
