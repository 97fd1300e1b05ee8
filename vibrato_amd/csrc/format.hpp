// User-defined output formats (MeCab's --node-format / --unk-format / --bos-format / --eos-format): what the
// host-side compiler (format.cpp), the engine (engine.hip: class Format) and the kernels (format.hip) share -- the op program a
// format string compiles to and the per-format field index on the device.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <mutex>
#include <string>
#include <string_view>
#include <vector>

#include "engine.hpp"

namespace vbt {

constexpr uint32_t kFmtMaxOps = 32, kFmtMaxSlots = 16, kFmtMaxLit = 256, kFmtMaxField = 255;

// One op = one u32: kind | x << 8 | y << 20 (x, y: 12 bits each).
//   kFmtLit:   x = where its bytes start in the string's literal pool, y = how many (1 .. 256)
//   kFmtField: x = slot | separator byte << 4, y = kFmtSep (a separator goes in front) | kFmtSkip (%F: an absent field or "*" prints
//              nothing, and the separator only goes between two fields that were printed) | kFmtFirst (the first index of its list)
//   the numeric kinds kFmtLeft .. kFmtLen are consecutive: kind - kFmtLeft is the nibble of a token's packed widths
// Every index of a %f / %F list is an op of its own (the commas of a %f list are its ops' separators, not literals).
enum FmtKind : uint32_t { kFmtLit = 0, kFmtSurface, kFmtFeature, kFmtField, kFmtIsUnk, kFmtLeft, kFmtRight, kFmtWordCost, kFmtTotalCost, kFmtStart, kFmtEnd, kFmtLen };
enum FmtFieldFlag : uint32_t { kFmtSep = 1, kFmtSkip = 2, kFmtFirst = 4 };
// FmtProgram::uses: what a token's ops read besides the staged record
enum FmtUses : uint32_t { kFmtUsesParams = 1, kFmtUsesNumbers = 2, kFmtUsesFeature = 4 };

// A compiled format as the kernels read it (a kernel argument, copied into LDS once per workgroup): programs and literal pools of the
// node format [0] and the unknown-word format [1], the bytes of bos and eos.
struct FmtProgram {
    uint32_t ops[2][kFmtMaxOps];
    uint8_t lit[2][kFmtMaxLit];
    uint8_t bos[kFmtMaxLit], eos[kFmtMaxLit];
    uint32_t n_ops[2];
    uint32_t bos_len, eos_len;
    uint32_t slots;  // distinct field indices of both programs
    uint32_t uses;
    uint8_t field[kFmtMaxSlots];  // slot -> CSV field index
};
static_assert(sizeof(FmtProgram) % 4 == 0, "copied as dwords");

// vbt_format_check / vbt_format_new: the four strings -> a program; VBT_ERR_INVALID_ARGUMENT names the string and the position
FmtProgram compile_format(std::string_view node, const char* unk /* nullptr: = node */, std::string_view bos, std::string_view eos);

// An entry of the field index: where the field's content lies and how long it is.  len == kFmtAbsent: the row has no such field;
// kFmtStar: the content is exactly "*"; kFmtSide: off counts into the format's side blob (a row the host parsed), not the feature blob.
constexpr uint32_t kFmtAbsent = 0xFFFFFFFFu, kFmtStar = 0x80000000u, kFmtSide = 0x40000000u, kFmtLenMask = 0x3FFFFFFFu;

// What the kernels of a format read (passed by value: the program travels in the kernel arguments): the program, and per word
// (row base[lex] + id of DevFeatures::off) `slots` index entries.
struct DevFormat {
    FmtProgram prog;
    const uint2* index;   // [rows][slots] {off, len}
    const uint8_t* side;  // field contents of the rows the host parsed + 8 zero bytes
};

// A compiled format of one tokenizer (vbt_format).  The device side -- the program and the field index, which format_index cuts
// out of the feature blob that is already in HBM -- is built under a call_once at first use and freed with the object (the tokenizer must outlive it only as far as its use goes: the destructor frees by device ordinal); a failed
// build frees what it allocated and is tried again by the next call.  Independent of the renumbering of the connection ids.
class Format {
  public:
    Format(const Tokenizer& tok, const FmtProgram& prog) : tok(tok), prog(prog), device_(tok.device()) {}
    ~Format();
    Format(const Format&) = delete;
    Format& operator=(const Format&) = delete;
    const DevFormat& device() const;
    const Tokenizer& tok;
    const FmtProgram prog;
    // bytes of output per KiB of text, the largest seen: the first capacity of vbt_tokenize_format
    mutable std::atomic<uint32_t> per_kib{0};

  private:
    mutable std::once_flag once_;
    mutable DevFormat dev_{prog, nullptr, nullptr};
    mutable void* allocs_[2] = {nullptr, nullptr};
    const int device_;  // the tokenizer's device: the destructor does not reach for the tokenizer
};

}  // namespace vbt
