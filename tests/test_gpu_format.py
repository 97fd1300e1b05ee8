"""User-defined output formats rendered on the device (format.hip) against a plain formatter over the oracle's tokens, byte for byte:
Tokenizer.compile_format / tokenize_format, and the format compiler's refusals (vbt_format_check, which needs no device)."""
import csv
import functools
import re

import numpy as np
import pytest

import vibrato_amd as V
from vibrato_amd.api import format_check
from oracle import oracle as ora
from tools import synth

gpu = pytest.mark.gpu
R = V.FORMAT_ROUND
SENTS = ["京都東京都京都", "kampersanda", "", "東京県に行く", "一橋大学大学院", "東京 都", "  ", " 東京  都 ", "𠮷野家"]  # (test_gpu_detail.py's + a 4-byte character)
DIRECTIVE = re.compile(r"%(phl|phr|pw|pc|ps|pe|pl|[mHcs%]|f|F(.))(?:\[([\d,]+)\])?", re.S)


def _expand(fmt, t):
    """one token in the format `fmt`: the directive table of include/vibrato_hip.h over the oracle's token dict"""
    fields = next(csv.reader([t["feature"]]), None) or [""]
    (ps, pe), wc = t["range_byte"], t["word_cost"]
    num = {"phl": t["left_id"], "phr": t["right_id"], "pw": wc, "c": wc, "pc": t["total_cost"], "ps": ps, "pe": pe, "pl": pe - ps, "s": int(t["lex_type"] == 2)}

    def one(m):
        d, sep, idx = m.group(1), m.group(2), [int(i) for i in (m.group(3) or "").split(",") if i]
        if d[0] == "f":
            return ",".join(fields[i] if i < len(fields) else "" for i in idx)
        if d[0] == "F":
            return sep.join(fields[i] for i in idx if i < len(fields) and fields[i] != "*")
        return {"m": t["surface"], "H": t["feature"], "%": "%"}[d] if d in "mH%" else str(num[d])
    return DIRECTIVE.sub(one, fmt)


def _lines(to, sents, node, unk=None, bos="", eos="EOS\n"):
    """per sentence (its expected line, its tokens)"""
    w, out = to.new_worker(), []
    for x in sents:
        w.reset_sentence(x)
        w.tokenize()
        toks = [w.token(i) for i in range(w.num_tokens())]
        out.append(((bos + "".join(_expand(unk if unk is not None and t["lex_type"] == 2 else node, t) for t in toks) + eos).encode(), len(toks)))
    return out


def _check(tv, sents, exp, node, **kw):
    """tokenize_format of `sents` == the expected lines, and line_off == the prefix of their lengths"""
    got, off = tv.tokenize_format(sents, tv.compile_format(node, **kw), with_offsets=True)
    assert got == b"".join(exp)
    assert off.tolist() == np.cumsum([0] + [len(e) for e in exp]).tolist()


@gpu
@pytest.mark.parametrize("ignore_space,max_grouping_len", [(False, 0), (True, 24)])
@pytest.mark.parametrize("node,kw", [("%m\t%H\n", {}), ("%f[0],%F/[1,2,3,9]|%m\n", {"unk": "?%m\n"}), ("%phl %phr %pw %pc %ps %pe %pl %s%%\n", {}),
                                     ("%m ", {"bos": "<s>", "eos": "\n"})], ids=["mecab", "fields", "numbers", "bos-eos"])
def test_fixture_sentences(fixture_sources, node, kw, ignore_space, max_grouping_len):
    """system, user and unknown words; empty lines and lines of spaces (bos + eos alone), skipped spaces, 3- and 4-byte characters"""
    s = fixture_sources
    d = V.SystemDictionaryBuilder.from_readers(s["lex.csv"], s["matrix.def"], s["char.def"], s["unk.def"])
    d.reset_user_lexicon_from_reader(s["user.csv"])
    do = ora.Dictionary.from_sources(s["lex.csv"], s["matrix.def"], s["char.def"], s["unk.def"]).reset_user_lexicon(s["user.csv"])
    to, tv = ora.Tokenizer(do, ignore_space, max_grouping_len), V.Tokenizer(d).ignore_space(ignore_space).max_grouping_len(max_grouping_len)
    exp = [ln for ln, _ in _lines(to, SENTS, node, **kw)]
    _check(tv, SENTS, exp, node, **kw)
    if node == "%m\t%H\n":
        assert b"".join(exp) == tv.tokenize_mecab(SENTS) == tv.tokenize_format(SENTS, node)  # (a str: compiled and kept by the tokenizer)


PIECES = "%m|%f[0]|%f[1,4]|%F/[1,2,3,9]|%H|%phl,%phr,%pw,%pc,%ps,%pe,%pl,%s lits\n"


@functools.lru_cache(maxsize=None)
def _piece_case(side):
    """eight one-character words as test_gpu_detail.py's _width_case has them -- ids on `side` 1 .. 5 digits wide, word costs of every
    width and both signs -- whose features have fields of 0 .. 7 bytes, a "*", a quoted field with a comma, one with a doubled quote,
    one with bytes behind its closing quote (the last two: rows the host parses) and fewer fields than PIECES asks for; three 29-byte
    lines ("a||,|||1,0,0,0,0,1,1,0 lits\\n\\n") in front of eight sentences of all the words in every cyclic order"""
    chars, ids, costs = "abcdeあいう", [1, 10, 100, 1000, 10000, 9, 99, 54321], [0, 9, 10, -1, -9, -10, 32767, -32768]
    feats = ["", "F", "FF,*,G", 'FFF,"x,y",HH,*', 'FFFF,"q""r",I', "FFFFF,GGGGGG,HHHHHHH,,J", '*,"z"w,K', "FFFFFFF,AB,CDE,FGHI,JKLMN,,,,,OPQRSTU"]
    lex = "".join(f"{c},{i if side == 'left' else 0},{i if side == 'right' else 0},{w},{f}\n" for c, i, w, f in zip(chars, ids, costs, feats)).encode()
    wide, dims = np.zeros(54322, dtype=np.int16), ((1, 54322) if side == "left" else (54322, 1))  # (num_right, num_left)
    src = (lex, wide, *dims, b"DEFAULT 0 1 0\n", b"DEFAULT,0,0,100,*\n")
    to = ora.Tokenizer(ora.Dictionary.from_sources_binmatrix(*src), False, 0)
    sents = ["a"] * 3 + [chars[k:] + chars[:k] for k in range(8)]
    return V.Tokenizer(V.SystemDictionaryBuilder.from_readers_binmatrix(*src)), sents, [ln for ln, _ in _lines(to, sents, PIECES, eos="\n")]


@gpu
@pytest.mark.parametrize("r", [0, 1, 2, 3])
@pytest.mark.parametrize("side", ["left", "right"])
def test_every_piece_kind_at_every_alignment(side, r):
    """dropping r of the three leading lines moves everything behind them by r bytes mod 4: every piece meets every alignment"""
    tv, sents, exp = _piece_case(side)
    assert [len(e) % 4 for e in exp[:3]] == [1, 1, 1]
    assert all(x in exp[3] for x in (b"|x,y,|x,y/HH|", b'|q"r,|q"r/I|', b"|zw,|zw/K|", b"|GGGGGG/HHHHHHH/|", b"|AB/CDE/FGHI/OPQRSTU|", b"-32768"))
    _check(tv, sents[r:], exp[r:], PIECES, eos="\n")


@functools.lru_cache(maxsize=None)
def _synth(shape, n, law="uniform_5_20"):
    sd = synth.SynthDict(shape)
    do = ora.Dictionary.from_sources_binmatrix(sd.lex, sd.matrix, sd.num_right, sd.num_left, sd.char_def, sd.unk)
    dv = V.SystemDictionaryBuilder.from_readers_binmatrix(sd.lex, sd.matrix, sd.num_right, sd.num_left, sd.char_def, sd.unk)
    text, offs = sd.sentences(n, law)
    return ora.Tokenizer(do, False, 0), V.Tokenizer(dv), [bytes(text[offs[i]:offs[i + 1]]) for i in range(n)], (text, offs)


BORDERS = "%m/%f[1]/%pc\t%H\n"


@gpu
@pytest.mark.parametrize("count", [R - 1, R, R + 1, 2 * R + 1])
def test_round_borders(count):
    """one sentence of exactly `count` tokens (by the oracle): the first sentence of the corpus repeated, cut where the oracle counts that many"""
    to, tv, sents, _ = _synth("tiny", 257)
    chars = sents[0].decode() * (2 * R + 2)
    for k in range(count, len(chars)):
        (line, ntok), = _lines(to, [chars[:k]], BORDERS)
        if ntok >= count:
            break
    assert ntok == count
    _check(tv, [chars[:k]], [line], BORDERS)


@gpu
def test_tile_border():
    to, tv, sents, _ = _synth("tiny", 257)
    _check(tv, sents, [ln for ln, _ in _lines(to, sents, BORDERS, bos="^")], BORDERS, bos="^")


@gpu
def test_ten_digit_totals_of_both_signs():
    """test_gpu_detail.py's Raw connector: 1000 x "a" ends at 1 998 000 000, 1025 x "b" at INT32_MIN"""
    src = (b"a,1,1,0,x\nb,2,2,0,y\n", "1\tRA\n2\tRB\n", "1\tLA\n2\tLB\n", "RA/LA\t2000000\nRB/LB\t-2097152\n", b"DEFAULT 0 1 0\n", b"DEFAULT,0,0,0,*\n")
    to = ora.Tokenizer(ora.Dictionary.from_sources_bigram(*src), False, 0)
    sents = ["a" * 1000, "b" * 1025, "ab" * 40, ""]
    exp = [ln for ln, _ in _lines(to, sents, "%pc %pe\n")]
    assert b"1998000000 1000\n" in exp[0] and b"-2147483648 1025\n" in exp[1]
    _check(V.Tokenizer(V.SystemDictionaryBuilder.from_readers_with_bigram_info(*src)), sents, exp, "%pc %pe\n")


@gpu
def test_host_call_regrows_once(monkeypatch):
    to, tv, sents, _ = _synth("tiny", 257)
    exp = [ln for ln, _ in _lines(to, sents, BORDERS)]
    monkeypatch.setenv("VBT_FORMAT_FIRST_CAP", "16")
    _check(tv, sents, exp, BORDERS)
    monkeypatch.delenv("VBT_FORMAT_FIRST_CAP")
    _check(tv, sents, exp, BORDERS)


@gpu
def test_dictionary_ids_after_the_device_ids_were_renumbered():
    to, tv, sents, (text, offs) = _synth("small", 4000, "lognormal_40")
    info = tv.calibrate(text=text, offsets=offs)
    assert info["state"] == "done" and info["moved_left"] + info["moved_right"] > 0
    _check(tv, sents[:300], [ln for ln, _ in _lines(to, sents[:300], "%phl %phr\n")], "%phl %phr\n")


@gpu
def test_cli_node_unk_bos_eos_formats(tmp_path, fixture_sources):
    """-F -U -B with the default -E, the escapes as a shell hands them over, on the fixture dictionary as a directory of sources"""
    import io
    from vibrato_amd import cli
    s = fixture_sources
    for k in ("lex.csv", "matrix.def", "char.def", "unk.def"):
        (tmp_path / k).write_bytes(s[k])
    to = ora.Tokenizer(ora.Dictionary.from_sources(s["lex.csv"], s["matrix.def"], s["char.def"], s["unk.def"]), False, 0)
    out = io.BytesIO()
    cli.main(["-i", str(tmp_path), "-F", "%m\\t%f[0]\\n", "-U", "%m\\t?\\n", "-B", "<s>\\n"], stdin=io.BytesIO("\n".join(SENTS).encode() + b"\n"), stdout=out)
    assert out.getvalue() == b"".join(ln for ln, _ in _lines(to, SENTS, "%m\t%f[0]\n", unk="%m\t?\n", bos="<s>\n"))


@pytest.mark.parametrize("kw", [{"node": "%q"}, {"node": "%f[1,2"}, {"node": "%f[" + ",".join(map(str, range(17))) + "]"}, {"node": "%m" * 33},
                                {"node": "%m", "eos": "%m\n"}, {"node": "%f[256]"}, {"node": "%f[]"}],
                         ids=["directive", "unterminated", "17-fields", "33-ops", "directive-in-eos", "field-256", "empty-list"])
def test_malformed_formats_are_refused(kw):
    format_check("%m\t%f[0,255]%F-[1]\\n", unk="%%", bos="\\0", eos="")  # (a good one passes)
    with pytest.raises(V.VibratoError) as e:
        format_check(**kw)
    assert e.value.code == 1 and "position" in e.value.message
