"""Wakati output rendered on the device (wakati.hip) against the oracle's formatter, byte for byte: Tokenizer.tokenize_wakati and
the device-resident Workspace.set_wakati / wakati_ptrs."""
import functools

import numpy as np
import pytest

import vibrato_amd as V
from vibrato_amd import sharding
from oracle import oracle as ora
from tools import synth

pytestmark = pytest.mark.gpu
R = V.WAKATI_ROUND
SENTS = ["京都東京都京都", "kampersanda", "", "東京県に行く", "一橋大学大学院", "東京 都", "  ", " 東京  都 "]


def _lines(to, sents):
    w, out = to.new_worker(), []
    for x in sents:
        w.reset_sentence(x)
        w.tokenize()
        out.append((ora.format_tokens(w, "wakati").encode(), w.num_tokens()))
    return out


def _check(tv, sents, exp):
    """tokenize_wakati of `sents` == the expected lines, and line_off == the prefix of their lengths"""
    got, off = tv.tokenize_wakati(sents, with_offsets=True)
    assert got == b"".join(exp)
    assert off.tolist() == np.cumsum([0] + [len(e) for e in exp]).tolist()


@functools.lru_cache(maxsize=None)
def _synth(shape, ignore_space, n, law="uniform_5_20", space_p=0.3):
    """(oracle tokenizer, product tokenizer, sentences, the oracle's wakati lines) on a synthetic dictionary: computed once"""
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
    """empty lines, a sentence of spaces only, skipped spaces at the head / middle / tail, 3- and 4-byte characters, every line alignment"""
    s = fixture_sources
    d = V.SystemDictionaryBuilder.from_readers(s["lex.csv"], s["matrix.def"], s["char.def"], s["unk.def"])
    d.reset_user_lexicon_from_reader(s["user.csv"])
    do = ora.Dictionary.from_sources(s["lex.csv"], s["matrix.def"], s["char.def"], s["unk.def"]).reset_user_lexicon(s["user.csv"])
    tv = V.Tokenizer(d).ignore_space(ignore_space).max_grouping_len(max_grouping_len)
    _check(tv, sents, [ln for ln, _ in _lines(ora.Tokenizer(do, ignore_space, max_grouping_len), sents)])


@pytest.mark.parametrize("ignore_space", [False, True])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_tile_borders(n, ignore_space):
    _, tv, sents, exp = _synth("tiny", ignore_space, 513)
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
    """a sentence swept in segments whose staging region and line exceed 16-bit sizes; reference: the host formatter (pinned to the oracle elsewhere)"""
    _, tv, sents, _ = _synth("small", False, 2000, "lognormal_40", 0.05)
    long = b"".join(sents[300:])[:70000].decode("utf-8", "ignore").encode()
    assert len(long) > 69990
    mixed = sents[:150] + [long] + sents[150:300]
    exp = tv.tokenize_batch(mixed).format("wakati").encode()
    got, off = tv.tokenize_wakati(mixed, with_offsets=True)
    assert got == exp and int(off[-1]) == len(exp) and int(off[151] - off[150]) > 70000


def test_device_api_window_records_and_capacity():
    """offsets[0] != 0; then the records next to the lines; then a capacity one byte short: flag 32, the lines in front of the
    failing one intact, nothing written from where it would have started to behind the buffer"""
    import torch
    to, tv, sents, exp = _synth("tiny", True, 513)
    n, pad = len(sents), 37
    text = np.frombuffer(b"x" * pad + b"".join(sents), dtype=np.uint8)
    offs = np.cumsum([pad] + [len(x) for x in sents]).astype(np.int64)
    d_text, d_offs = torch.from_numpy(text.copy()).cuda(), torch.from_numpy(offs).cuda()
    ws = tv.workspace(n, len(text))
    stream, total = torch.cuda.current_stream().cuda_stream, sum(len(e) for e in exp)

    def run(**kw):
        ws.set_wakati(True, **kw)
        ws.run(d_text.data_ptr(), d_offs.data_ptr(), n, len(text) - pad, stream)
        st, p = ws.stats(), ws.wakati_ptrs()
        return st, sharding.device_view(p["out"], total + 64, ws), sharding.device_view(p["line_off"], 8 * (n + 1), ws).cpu().numpy().view(np.uint64)

    st, out, off = run()
    assert st["error_flags"] == 0 and off.tolist() == np.cumsum([0] + [len(e) for e in exp]).tolist()
    assert out[:total].cpu().numpy().tobytes() == b"".join(exp)
    st, out, _ = run(keep_records=True)
    v = sharding.workspace_views(ws, n, st["n_tokens"])
    got, _ = sharding.tokens_in_sentence_order(*(v[k].cpu().numpy().view(t) for k, t in (("tok_off", np.uint32), ("tok_cnt", np.uint32), ("tokens", V.TOKEN_DTYPE))))
    ref, _ = to.new_worker().tokenize_batch(text[pad:], offs - pad)
    assert got.tobytes() == ref.tobytes() and out[:total].cpu().numpy().tobytes() == b"".join(exp)
    out.fill_(0xA5)
    torch.cuda.synchronize()
    st, out, off = run(_out_cap=total - 1)
    host = out.cpu().numpy().tobytes()
    assert st["error_flags"] == 32 and int(off[n]) == total
    assert host[:int(off[n - 1])] == b"".join(exp[:-1]) and host[int(off[n - 1]):] == b"\xa5" * (len(exp[-1]) + 64)


def test_multi_device_tokenizer_is_refused():
    sd = synth.SynthDict("tiny")
    dv = V.SystemDictionaryBuilder.from_readers_binmatrix(sd.lex, sd.matrix, sd.num_right, sd.num_left, sd.char_def, sd.unk)
    with pytest.raises(V.VibratoError) as e:
        V.Tokenizer(dv, devices=[0, 0]).tokenize_wakati(["abc"])
    assert e.value.code == 101
