// The format language of vbt_format_new / vbt_format_check (MeCab's --node-format family): four strings compiled
// into the op program format.hip interprets.  Pure host code: no device is touched.
#include <cstring>

#include "format.hpp"

namespace vbt {
namespace {

struct Builder {
    FmtProgram& p;
    const char* name;  // of the string being compiled, for messages
    int which;         // 0 node, 1 unk; -1: bos / eos (literals only)
    uint8_t* lit;
    uint32_t lit_len = 0, lit_open = 0;  // bytes in the pool; bytes of the literal op that is still growing
    uint32_t n_ops = 0;

    [[noreturn]] void fail(size_t at, const std::string& what) const {
        throw Error(VBT_ERR_INVALID_ARGUMENT, std::string(name) + " format, position " + std::to_string(at) + ": " + what);
    }
    void op(size_t at, uint32_t word) {
        if (which < 0) fail(at, "directives are not allowed in the bos and eos formats (literals, escapes and %% only)");
        if (n_ops == kFmtMaxOps) fail(at, "more than 32 ops");
        p.ops[which][n_ops++] = word;
        lit_open = 0;
    }
    void byte(size_t at, uint8_t c) {
        if (lit_len == kFmtMaxLit) fail(at, "more than 256 literal bytes");
        if (which >= 0) {
            if (lit_open) p.ops[which][n_ops - 1] += 1u << 20;  // one byte more
            else { op(at, kFmtLit | lit_len << 8 | 1u << 20); }
            lit_open = 1;
        }
        lit[lit_len++] = c;
    }
    uint32_t slot(size_t at, uint32_t field) {
        for (uint32_t s = 0; s < p.slots; ++s)
            if (p.field[s] == field) return s;
        if (p.slots == kFmtMaxSlots) fail(at, "more than 16 distinct field indices");
        p.field[p.slots] = (uint8_t)field;
        return p.slots++;
    }
    // "[i,j,...]" at s[pos]: one kFmtField op per index; returns the position behind ']'
    size_t list(std::string_view s, size_t pos, uint32_t sep, bool skip) {
        if (pos >= s.size() || s[pos] != '[') fail(pos, "'[' expected");
        const size_t open = pos++;
        bool first = true;
        for (;;) {
            size_t d = pos;
            uint32_t v = 0;
            while (d < s.size() && s[d] >= '0' && s[d] <= '9' && v <= kFmtMaxField) v = v * 10 + (uint32_t)(s[d++] - '0');
            if (d == pos) fail(pos, pos >= s.size() ? "unterminated '['" : first && s[pos] == ']' ? "empty index list" : "a field index expected");
            if (v > kFmtMaxField) fail(pos, "field index above 255");
            op(pos, kFmtField | (slot(pos, v) | sep << 4) << 8 | ((first ? kFmtFirst : kFmtSep) | (skip ? kFmtSkip : 0u)) << 20);
            first = false;
            pos = d;
            if (pos >= s.size()) fail(open, "unterminated '['");
            if (s[pos] == ']') return pos + 1;
            if (s[pos] != ',') fail(pos, "',' or ']' expected");
            ++pos;
        }
    }
    void compile(std::string_view s) {
        static const char esc_in[] = "0abtnvfr\\", esc_out[] = "\0\a\b\t\n\v\f\r\\";
        for (size_t i = 0; i < s.size();) {
            const char c = s[i];
            if (c == '\\') {
                const char* e = i + 1 < s.size() ? static_cast<const char*>(std::memchr(esc_in, s[i + 1], 9)) : nullptr;
                if (!e) fail(i, "unknown escape");
                byte(i, (uint8_t)esc_out[e - esc_in]);
                i += 2;
            } else if (c != '%') {
                byte(i, (uint8_t)c);
                ++i;
            } else {
                const std::string_view d = s.substr(i + 1);
                auto is = [&](const char* w) { return d.substr(0, std::strlen(w)) == w; };
                const size_t at = i;
                if (is("%")) { byte(at, '%'); i += 2; }
                else if (is("m")) { op(at, kFmtSurface); i += 2; }
                else if (is("H")) { op(at, kFmtFeature); p.uses |= kFmtUsesFeature; i += 2; }
                else if (is("f")) i = list(s, i + 2, ',', false);
                else if (is("F")) { if (i + 2 >= s.size()) fail(at, "%F needs a separator byte"); i = list(s, i + 3, (uint8_t)s[i + 2], true); }
                else if (is("phl")) { op(at, kFmtLeft); p.uses |= kFmtUsesParams | kFmtUsesNumbers; i += 4; }
                else if (is("phr")) { op(at, kFmtRight); p.uses |= kFmtUsesParams | kFmtUsesNumbers; i += 4; }
                else if (is("pw")) { op(at, kFmtWordCost); p.uses |= kFmtUsesParams | kFmtUsesNumbers; i += 3; }
                else if (is("pc")) { op(at, kFmtTotalCost); p.uses |= kFmtUsesNumbers; i += 3; }
                else if (is("ps")) { op(at, kFmtStart); p.uses |= kFmtUsesNumbers; i += 3; }
                else if (is("pe")) { op(at, kFmtEnd); p.uses |= kFmtUsesNumbers; i += 3; }
                else if (is("pl")) { op(at, kFmtLen); p.uses |= kFmtUsesNumbers; i += 3; }
                else if (is("c")) { op(at, kFmtWordCost); p.uses |= kFmtUsesParams | kFmtUsesNumbers; i += 2; }
                else if (is("s")) { op(at, kFmtIsUnk); i += 2; }
                else fail(at, "unknown directive");
            }
        }
    }
};

}  // namespace

FmtProgram compile_format(std::string_view node, const char* unk, std::string_view bos, std::string_view eos) {
    FmtProgram p{};
    Builder n{p, "node", 0, p.lit[0]};
    n.compile(node);
    p.n_ops[0] = n.n_ops;
    Builder u{p, "unk", 1, p.lit[1]};
    u.compile(unk ? std::string_view(unk) : node);
    p.n_ops[1] = u.n_ops;
    Builder b{p, "bos", -1, p.bos};
    b.compile(bos);
    p.bos_len = b.lit_len;
    Builder e{p, "eos", -1, p.eos};
    e.compile(eos);
    p.eos_len = e.lit_len;
    return p;
}

}  // namespace vbt
