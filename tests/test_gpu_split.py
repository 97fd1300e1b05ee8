"""Lines cut on the device (split.hip): Tokenizer.split_lines against five lines of Python, Tokenizer.tokenize_stream against the
text entry points fed with those lines."""
import functools

import pytest

import vibrato_amd as V
from tools import synth
from tests.test_gpu_wakati import SENTS

pytestmark = pytest.mark.gpu
T = V.SPLIT_TILE
FILL = bytes(range(0x20, 0x7F))  # no '\r', no '\n', period 95: a shifted copy is a different text


def ref(raw, final):
    parts = raw.split(b"\n"); tail = parts.pop()
    lines = [p[:-1] if p.endswith(b"\r") else p for p in parts]
    if final and tail: lines.append(tail)
    return lines, (len(raw) if final else len(raw) - len(tail))


def buf(n, *marks):
    """n filler bytes with `bytes` written over them at `position`, for every (position, bytes) of marks"""
    b = bytearray((FILL * (n // len(FILL) + 1))[:n])
    for at, what in marks:
        b[at:at + len(what)] = what
    return bytes(b)


KYO = "京".encode()
CASES = {**{repr(c): c for c in [b"", b"\n", b"a", b"a\n", b"a\r\n", b"a\r", b"\r\n", b"\r\r\n", b"a\rb\n", b"\n\n\n"]},
         "no newline": buf(300), "T+1 newlines": b"\n" * (T + 1),
         **{f"one line of {n}": buf(n) for n in (T - 1, T, T + 1, 2 * T + 3)},
         **{f"nl at {p}": buf(T + 40, (p, b"\n")) for p in (T - 1, T)},
         **{f"crnl at {p}": buf(T + 40, (7, b"\r"), (p, b"\r\n"), (p + 9, b"\r")) for p in (15, 64 * 16 - 1, T - 2, T - 1, T)},
         "kyo over T, 1 dropped": buf(T + 40, (5, b"\n"), (T - 1, KYO)), "kyo over T, 2 dropped": buf(T + 40, (5, b"\r\n"), (T - 2, KYO))}


@functools.lru_cache(maxsize=None)
def _tiny():
    """(tokenizer on the `tiny` synthetic dictionary, 513 of its sentences joined by '\\n')"""
    sd = synth.SynthDict("tiny")
    tv = V.Tokenizer(V.SystemDictionaryBuilder.from_readers_binmatrix(sd.lex, sd.matrix, sd.num_right, sd.num_left, sd.char_def, sd.unk))
    text, offs = sd.sentences(513, "uniform_5_20", space_p=0.3)
    raw = b"\n".join(bytes(text[offs[i]:offs[i + 1]]) for i in range(513))
    assert raw.count(b"\n") == 512 and b"\r" not in raw and len(raw) > T + 7
    return tv, raw


@pytest.mark.parametrize("final", [True, False])
@pytest.mark.parametrize("raw", CASES.values(), ids=CASES.keys())
def test_split_lines(raw, final):
    lines, consumed = ref(raw, final)
    text, offsets, used = _tiny()[0].split_lines(raw, final)
    assert used == consumed and len(offsets) == len(lines) + 1
    assert [text[offsets[i]:offsets[i + 1]] for i in range(len(lines))] == lines and offsets[0] == 0 and offsets[-1] == len(text)


@pytest.mark.parametrize("mode", ["mecab", "wakati", "detail"])
@pytest.mark.parametrize("sep,end", [(b"\n", b""), (b"\n", b"\n"), (b"\r\n", b""), (b"\r\n", b"\r\n")])
def test_stream_fixture_sentences(fixture_sources, mode, sep, end):
    s = fixture_sources
    tv = V.Tokenizer(V.SystemDictionaryBuilder.from_readers(s["lex.csv"], s["matrix.def"], s["char.def"], s["unk.def"]))
    raw = sep.join(x.encode() for x in SENTS) + end
    lines = ref(raw, True)[0]
    assert tv.tokenize_stream(raw, mode) == (getattr(tv, "tokenize_" + mode)(lines), len(lines), len(raw))


@pytest.mark.parametrize("mode", ["mecab", "wakati", "detail"])
def test_stream_in_one_call_and_in_pieces(mode):
    tv, raw = _tiny()
    whole = getattr(tv, "tokenize_" + mode)(ref(raw, True)[0])
    assert tv.tokenize_stream(raw, mode) == (whole, 513, len(raw))
    got, carry = b"", b""
    for at in range(0, len(raw), T + 7):
        carry += raw[at:at + T + 7]
        out, _, used = tv.tokenize_stream(carry, mode, final=False)
        got, carry = got + out, carry[used:]
    assert got + tv.tokenize_stream(carry, mode, final=True)[0] == whole
    assert tv.tokenize_stream(raw[:20].replace(b"\n", b" "), mode, final=False) == (b"", 0, 0)


@pytest.mark.parametrize("devices,raw,code", [(None, b"abc\n\xE3\x81\nabc\n", 5), ([0, 0], b"abc\n", 101)], ids=["utf8", "multi-device"])
def test_errors(devices, raw, code):
    sd = synth.SynthDict("tiny")
    dv = V.SystemDictionaryBuilder.from_readers_binmatrix(sd.lex, sd.matrix, sd.num_right, sd.num_left, sd.char_def, sd.unk)
    with pytest.raises(V.VibratoError) as e:
        (V.Tokenizer(dv, devices=devices) if devices else V.Tokenizer(dv)).tokenize_stream(raw)
    assert e.value.code == code and (code != 5 or "line 1 " in e.value.message)
