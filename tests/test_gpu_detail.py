"""Detail output rendered on the device (detail.hip) against the oracle's formatter, byte for byte: Tokenizer.tokenize_detail and the
device-resident Workspace.set_detail / detail_ptrs / render_again."""
import functools
import re

import numpy as np
import pytest

import vibrato_amd as V
from vibrato_amd import sharding
from oracle import oracle as ora
from tools import synth

pytestmark = pytest.mark.gpu
R = V.DETAIL_ROUND
SENTS = ["京都東京都京都", "kampersanda", "", "東京県に行く", "一橋大学大学院", "東京 都", "  ", " 東京  都 "]  # (the list of test_gpu_wakati.py)


def _lines(to, sents):
    w, out = to.new_worker(), []
    for x in sents:
        w.reset_sentence(x)
        w.tokenize()
        out.append((ora.format_tokens(w, "detail").encode(), w.num_tokens()))
    return out


def _prefix(exp):
    return np.cumsum([0] + [len(e) for e in exp]).tolist()


def _check(tv, sents, exp):
    """tokenize_detail of `sents` == the expected lines, and line_off == the prefix of their lengths"""
    got, off = tv.tokenize_detail(sents, with_offsets=True)
    assert got == b"".join(exp)
    assert off.tolist() == _prefix(exp)


def _fields(exp, name):
    return [int(v) for v in re.findall(rb"\t" + name + rb"=(-?\d+)", b"".join(exp))]


@functools.lru_cache(maxsize=None)
def _synth(shape, ignore_space, n, law="uniform_5_20", space_p=0.3):
    """(oracle tokenizer, product tokenizer, sentences, the oracle's detail lines) on a synthetic dictionary: computed once"""
    sd = synth.SynthDict(shape)
    do = ora.Dictionary.from_sources_binmatrix(sd.lex, sd.matrix, sd.num_right, sd.num_left, sd.char_def, sd.unk)
    dv = V.SystemDictionaryBuilder.from_readers_binmatrix(sd.lex, sd.matrix, sd.num_right, sd.num_left, sd.char_def, sd.unk)
    to, tv = ora.Tokenizer(do, ignore_space, 0), V.Tokenizer(dv).ignore_space(ignore_space)
    text, offs = sd.sentences(n, law, space_p=space_p)
    sents = [bytes(text[offs[i]:offs[i + 1]]) for i in range(n)]
    return to, tv, sents, [ln for ln, _ in _lines(to, sents)]


@pytest.mark.parametrize("ignore_space,max_grouping_len", [(False, 0), (True, 24)])
@pytest.mark.parametrize("sents", [SENTS, ["𠮷野家"]], ids=["lines", "4-byte"])
def test_fixture_sentences(fixture_sources, sents, ignore_space, max_grouping_len):
    """the three lex_type names; empty lines and lines of spaces ("EOS" alone), skipped spaces, 3- and 4-byte characters"""
    s = fixture_sources
    d = V.SystemDictionaryBuilder.from_readers(s["lex.csv"], s["matrix.def"], s["char.def"], s["unk.def"])
    d.reset_user_lexicon_from_reader(s["user.csv"])
    do = ora.Dictionary.from_sources(s["lex.csv"], s["matrix.def"], s["char.def"], s["unk.def"]).reset_user_lexicon(s["user.csv"])
    tv = V.Tokenizer(d).ignore_space(ignore_space).max_grouping_len(max_grouping_len)
    exp = [ln for ln, _ in _lines(ora.Tokenizer(do, ignore_space, max_grouping_len), sents)]
    if sents is SENTS:
        assert {m for m in re.findall(rb"lex_type=(\w+)", b"".join(exp))} == {b"System", b"User", b"Unknown"}
    _check(tv, sents, exp)


@functools.lru_cache(maxsize=None)
def _width_case(side):
    """eight one-character words (1- and 3-byte surfaces, features of 0 .. 7 bytes) whose ids on `side` are 1 .. 5 digits wide (the
    other side's are 0: a matrix of one row or one column of zeros) and whose word costs have every width and both signs; three
    69-byte lines ("a\\t\\tlex_type=System\\tleft_id=1\\tright_id=0\\tword_cost=0\\ttotal_cost=0\\nEOS\\n", or the ids swapped) in front of
    eight sentences of all the words in every cyclic order"""
    chars, ids, costs = "abcdeあいう", [1, 10, 100, 1000, 10000, 9, 99, 54321], [0, 9, 10, -1, -9, -10, 32767, -32768]
    lex = "".join(f"{c},{i if side == 'left' else 0},{i if side == 'right' else 0},{w},{'F' * k}\n" for k, (c, i, w) in enumerate(zip(chars, ids, costs))).encode()
    wide, dims = np.zeros(54322, dtype=np.int16), ((1, 54322) if side == "left" else (54322, 1))  # (num_right, num_left)
    src = (lex, wide, *dims, b"DEFAULT 0 1 0\n", b"DEFAULT,0,0,100,*\n")
    to = ora.Tokenizer(ora.Dictionary.from_sources_binmatrix(*src), False, 0)
    sents = ["a"] * 3 + [chars[k:] + chars[:k] for k in range(8)]
    return V.Tokenizer(V.SystemDictionaryBuilder.from_readers_binmatrix(*src)), sents, [ln for ln, _ in _lines(to, sents)], ids, costs


@pytest.mark.parametrize("r", [0, 1, 2, 3])
@pytest.mark.parametrize("side", ["left", "right"])
def test_every_decimal_width_at_every_alignment(side, r):
    """dropping r of the three leading lines moves everything behind them by r bytes mod 4: every field meets every alignment"""
    tv, sents, exp, ids, costs = _width_case(side)
    assert [len(e) % 4 for e in exp[:3]] == [1, 1, 1]
    assert set(_fields(exp, side.encode() + b"_id")) == set(ids) and {len(str(i)) for i in ids} == {1, 2, 3, 4, 5}
    assert set(_fields(exp, b"word_cost")) == set(costs)
    totals = _fields(exp, b"total_cost")
    assert min(totals) < 0 < max(totals) and 0 in totals
    _check(tv, sents[r:] + sents[:r], exp[r:] + exp[:r])


def test_ten_digit_totals_of_both_signs():
    """a Raw connector of two templates whose costs leave i16 by far: a -> a costs 2 000 000, b -> b costs -2^21.  1000 x "a" ends
    at 1 998 000 000; 1025 x "b" ends at 1024 x -2^21 = INT32_MIN, the one value whose magnitude is no i32"""
    src = (b"a,1,1,0,x\nb,2,2,0,y\n", "1\tRA\n2\tRB\n", "1\tLA\n2\tLB\n", "RA/LA\t2000000\nRB/LB\t-2097152\n", b"DEFAULT 0 1 0\n", b"DEFAULT,0,0,0,*\n")
    to = ora.Tokenizer(ora.Dictionary.from_sources_bigram(*src), False, 0)
    sents = ["a" * 1000, "b" * 1025, "ab" * 40, ""]
    exp = [ln for ln, _ in _lines(to, sents)]
    totals = _fields(exp, b"total_cost")
    assert max(totals) == 1998000000 and min(totals) == -2 ** 31 and {len(str(t)) for t in totals} >= {1, 7, 8, 10, 11}
    _check(V.Tokenizer(V.SystemDictionaryBuilder.from_readers_with_bigram_info(*src)), sents, exp)


def test_dictionary_ids_after_the_device_ids_were_renumbered():
    sd = synth.SynthDict("small")
    do = ora.Dictionary.from_sources_binmatrix(sd.lex, sd.matrix, sd.num_right, sd.num_left, sd.char_def, sd.unk)
    tv = V.Tokenizer(V.SystemDictionaryBuilder.from_readers_binmatrix(sd.lex, sd.matrix, sd.num_right, sd.num_left, sd.char_def, sd.unk))
    text, offs = sd.sentences(4000, "lognormal_40")
    info = tv.calibrate(text=text, offsets=offs)
    assert info["state"] == "done" and info["moved_left"] + info["moved_right"] > 0
    sents = [bytes(text[offs[i]:offs[i + 1]]) for i in range(300)]
    _check(tv, sents, [ln for ln, _ in _lines(ora.Tokenizer(do, False, 0), sents)])


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_tile_borders(n):
    _, tv, sents, exp = _synth("tiny", False, 513)
    _check(tv, sents[:n], exp[:n])


@pytest.mark.parametrize("count", [63, 64, 65, R - 1, R, R + 1])
def test_lane_and_round_borders(count):
    """one sentence of exactly `count` tokens (by the oracle): the first sentence of the corpus repeated, cut after the first
    character at which the oracle counts that many"""
    to, tv, sents, _ = _synth("tiny", False, 513)
    chars = sents[0].decode() * (R + 2)
    for k in range(count, len(chars)):
        (line, ntok), = _lines(to, [chars[:k]])
        if ntok >= count:
            break
    assert ntok == count
    _check(tv, [chars[:k]], [line])


def test_long_sentence_among_short_ones():
    """a sentence of more than 64 KiB, swept in segments; reference: the host formatter (pinned to the oracle elsewhere)"""
    _, tv, sents, _ = _synth("small", False, 2000, "lognormal_40", 0.05)
    long = b"".join(sents[300:])[:70000].decode("utf-8", "ignore").encode()
    assert len(long) > 69990
    mixed = sents[:150] + [long] + sents[150:300]
    exp = tv.tokenize_batch(mixed).format("detail").encode()
    got, off = tv.tokenize_detail(mixed, with_offsets=True)
    assert got == exp and int(off[-1]) == len(exp) and int(off[151] - off[150]) > 70000


def test_device_api_window_records_capacity_and_render_again():
    """offsets[0] != 0; then the records next to the lines; then a capacity one byte short: flag 32, line_off[n] the true total, the
    lines in front of the failing one intact, nothing written from where it would have started to behind the buffer's pad; then a
    larger buffer and render_again alone: no flag, the whole output"""
    import torch
    to, tv, sents, exp = _synth("tiny", True, 513)
    n, pad = len(sents), 37
    text = np.frombuffer(b"x" * pad + b"".join(sents), dtype=np.uint8)
    offs = np.cumsum([pad] + [len(x) for x in sents]).astype(np.int64)
    d_text, d_offs = torch.from_numpy(text.copy()).cuda(), torch.from_numpy(offs).cuda()
    ws = tv.workspace(n, len(text))
    stream, total = torch.cuda.current_stream().cuda_stream, sum(len(e) for e in exp)

    def result(cap):
        st, p = ws.stats(), ws.detail_ptrs()
        return st, sharding.device_view(p["out"], cap + 64, ws), sharding.device_view(p["line_off"], 8 * (n + 1), ws).cpu().numpy().view(np.uint64)

    def run(cap, **kw):
        ws.set_detail(True, cap_bytes=cap, **kw)
        ws.run(d_text.data_ptr(), d_offs.data_ptr(), n, len(text) - pad, stream)
        return result(cap)

    st, out, off = run(total)
    assert st["error_flags"] == 0 and off.tolist() == _prefix(exp)
    assert out[:total].cpu().numpy().tobytes() == b"".join(exp)
    st, out, _ = run(total, keep_records=True)
    v = sharding.workspace_views(ws, n, st["n_tokens"])
    got, _ = sharding.tokens_in_sentence_order(*(v[k].cpu().numpy().view(t) for k, t in (("tok_off", np.uint32), ("tok_cnt", np.uint32), ("tokens", V.TOKEN_DTYPE))))
    ref, _ = to.new_worker().tokenize_batch(text[pad:], offs - pad)
    assert got.tobytes() == ref.tobytes() and out[:total].cpu().numpy().tobytes() == b"".join(exp)
    out.fill_(0xA5)
    torch.cuda.synchronize()
    st, out, off = run(total - 1)
    host = out.cpu().numpy().tobytes()
    assert st["error_flags"] == 32 and int(off[n]) == total
    assert host[:int(off[n - 1])] == b"".join(exp[:-1]) and host[int(off[n - 1]):] == b"\xa5" * (len(exp[-1]) - 1 + 64)
    ws.set_detail(True, cap_bytes=total + 100)  # (more than the buffer holds: a new one, with nothing in it)
    ws.render_again(stream)
    st, out, off = result(total + 100)
    assert st["error_flags"] == 0 and off.tolist() == _prefix(exp)
    assert out[:total].cpu().numpy().tobytes() == b"".join(exp)


def test_host_call_regrows_once(monkeypatch):
    _, tv, sents, exp = _synth("tiny", False, 513)
    monkeypatch.setenv("VBT_DETAIL_FIRST_CAP", "16")
    _check(tv, sents, exp)
    monkeypatch.delenv("VBT_DETAIL_FIRST_CAP")
    _check(tv, sents, exp)


def test_refusals():
    """a multi-device tokenizer; each pair of the three text modes on one workspace, and the second mode once the first is off"""
    sd = synth.SynthDict("tiny")
    dv = V.SystemDictionaryBuilder.from_readers_binmatrix(sd.lex, sd.matrix, sd.num_right, sd.num_left, sd.char_def, sd.unk)
    with pytest.raises(V.VibratoError) as e:
        V.Tokenizer(dv, devices=[0, 0]).tokenize_detail(["abc"])
    assert e.value.code == 101
    ws = _synth("tiny", False, 513)[1].workspace(4, 64)
    modes = {"wakati": lambda on: ws.set_wakati(on), "mecab": lambda on: ws.set_mecab(on, cap_bytes=1024), "detail": lambda on: ws.set_detail(on, cap_bytes=1024)}
    for first in modes:
        for second in modes:
            if first != second:
                modes[first](True)
                with pytest.raises(V.VibratoError):
                    modes[second](True)
                modes[first](False)
                modes[second](True)
                modes[second](False)
