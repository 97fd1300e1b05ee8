"""Tokenizer.tokenize_nbest (MeCab's -N) on the GPU: against exhaustive enumeration on dictionaries whose lattice the host-side
accessors describe completely (every character a word, no unknown words, no user lexicon), and by properties elsewhere."""
import numpy as np
import pytest

import vibrato_amd as V
from tools import synth

pytestmark = pytest.mark.gpu

CHAR, UNK = "DEFAULT 0 1 0", "DEFAULT,0,0,0,*"
WORDS = [("a", 1, 1, 3), ("a", 2, 3, 1), ("b", 1, 2, 4), ("c", 3, 1, 2), ("ab", 2, 2, 5), ("ab", 3, 1, 6), ("bc", 1, 3, 7), ("ca", 2, 1, 5), ("abc", 3, 3, 9)]
SENTS = ["", "a", "ab", "abcab", "abcabcab"]


def _lex(words, zero=False):
    return "".join(f"{s},{l},{r},{0 if zero else c},f{i}\n" for i, (s, l, r, c) in enumerate(words))


def _matrix(zero=False):
    return "4 4\n" + "".join(f"{r} {l} {0 if zero else (3 * r + 5 * l + r * l) % 7 - 2}\n" for r in range(4) for l in range(4))


def _wide():
    """a Raw connector whose costs leave i16 (raw_connector.rs:153-161): i32 matrix cells on the device"""
    ids = "".join(f"{i}\tF{i}\n" for i in (1, 2, 3))
    cost = "".join(f"F{r}/F{l}\t{(r * 7 + l * 3) % 5 * 100000 - 150000}\n" for r in (1, 2, 3) for l in (1, 2, 3))
    return V.SystemDictionaryBuilder.from_readers_with_bigram_info(_lex(WORDS), ids, ids, cost, CHAR, UNK)


def _expected(d, text, n):
    """every path of the lattice, by DFS, in the contract's order: [(cost, [(start, end, word_id, total_cost)])]"""
    nodes, seq = [], 0
    for i in range(len(text)):
        row = []
        for wid, end, left, right, cost in d.common_prefix(text[i:]):
            row.append((seq, wid, i + end, left, right, cost))
            seq += 1
        nodes.append(row)
    paths = []

    def walk(pos, right, total, toks, seqs):
        if pos == len(text):
            paths.append((total + d.conn_cost(right, 0), tuple(-q for q in reversed(seqs)), toks))
            return
        for q, wid, end, left, r, cost in nodes[pos]:
            t = total + cost + d.conn_cost(right, left)
            walk(end, r, t, toks + [(pos, end, wid, t)], seqs + [q])

    if text:
        walk(0, 0, 0, [], [])
    assert len(paths) < 10 ** 5
    return [(c, toks) for c, _, toks in sorted(paths, key=lambda p: p[:2])[:n]]


def _check_exact(tv, sents, n):
    d, nb = tv.dictionary(), tv.tokenize_nbest(sents, n=n)
    for s, text in enumerate(sents):
        exp = _expected(d, text, n)
        assert nb.num_paths(s) == len(exp), (text, n)
        for r, (cost, toks) in enumerate(exp):
            got_cost, recs = nb.path(s, r)
            got = [(int(t["start_char"]), int(t["end_char"]), int(t["word_idx"]), int(t["total_cost"])) for t in recs]
            assert (got_cost, got) == (cost, toks), (text, n, r)
            assert (recs["start_byte"] == recs["start_char"]).all() and (recs["end_byte"] == recs["end_char"]).all()
    return nb


@pytest.mark.parametrize("n", [1, 2, 3, 16])
@pytest.mark.parametrize("kind", ["varied", "zero", "slab", "wide"])
def test_against_enumeration(kind, n, monkeypatch):
    """varied costs; all-zero costs (the tie rule alone); everything in the slab tier; i32 matrix cells"""
    if kind == "slab":
        monkeypatch.setenv("VBT_NBEST_LDS_KB", "0")
    zero = kind == "zero"
    d = _wide() if kind == "wide" else V.SystemDictionaryBuilder.from_readers(_lex(WORDS, zero), _matrix(zero), CHAR, UNK)
    nb = _check_exact(V.Tokenizer(d), SENTS, n)
    assert nb.slab_sentences() == (len(SENTS) - 1 if kind == "slab" else 0)


@pytest.mark.parametrize("h", [15, 16, 17, 65, 300])
def test_row_and_lane_borders(h):
    """h homographs of "a", many ties: steps with more predecessors than a row has lanes (h > 16) or than a chunk holds (h > 256),
    and more candidates than a wave has rows"""
    d = V.SystemDictionaryBuilder.from_readers(_lex([("a", 1 + i % 3, 1 + i % 2, i % 4) for i in range(h)]), _matrix(), CHAR, UNK)
    _check_exact(V.Tokenizer(d), ["aa"], 16)


def _check_properties(tv, sents, n):
    d, nb, one = tv.dictionary(), tv.tokenize_nbest(sents, n=n), tv.tokenize_batch(sents)
    path_off, tok_off, costs, toks = nb.arrays()
    assert path_off[0] == 0 and tok_off[0] == 0 and (np.diff(path_off.astype(np.int64)) >= 0).all() and (np.diff(tok_off.astype(np.int64)) >= 0).all()
    assert path_off[-1] == len(costs) == len(tok_off) - 1 and tok_off[-1] == len(toks)
    param, conn = {}, {}
    for s, text in enumerate(sents):
        text = text if isinstance(text, bytes) else text.encode()
        p0, p1 = int(path_off[s]), int(path_off[s + 1])
        assert p1 - p0 == nb.num_paths(s) <= n and (p1 > p0) == (len(text) > 0)
        seen = set()
        for p in range(p0, p1):
            recs = toks[int(tok_off[p]):int(tok_off[p + 1])]
            if p == p0:
                assert recs.tobytes() == one.records(s).tobytes()
            else:
                assert costs[p] >= costs[p - 1]
            seen.add(recs[["start_char", "word_idx"]].tobytes())
            right, total, at = 0, 0, 0
            for t in recs:
                w = int(t["word_idx"])
                left, r, wc = param.setdefault(w, d.word_param(w >> 30, w & 0x3FFFFFFF))
                total += wc + conn.setdefault((right, left), d.conn_cost(right, left))
                assert total == t["total_cost"] and (t["start_byte"] == at or text[at:t["start_byte"]].decode().isspace())
                right, at = r, int(t["end_byte"])
            assert total + conn.setdefault((right, 0), d.conn_cost(right, 0)) == costs[p] == nb.path(s, p - p0)[0]
            assert at == len(text) or text[at:].decode().isspace()
        assert len(seen) == p1 - p0
    return nb


def _tiny(ignore_space=False, max_grouping_len=0):
    sd = synth.SynthDict("tiny")
    dv = V.SystemDictionaryBuilder.from_readers_binmatrix(sd.lex, sd.matrix, sd.num_right, sd.num_left, sd.char_def, sd.unk)
    text, offs = sd.sentences(513, "uniform_5_20", space_p=0.3)
    return V.Tokenizer(dv).ignore_space(ignore_space).max_grouping_len(max_grouping_len), [bytes(text[offs[i]:offs[i + 1]]) for i in range(513)]


@pytest.mark.parametrize("ignore_space", [False, True])
@pytest.mark.parametrize("max_grouping_len", [0, 24])
def test_properties_on_the_synthetic_dictionary(ignore_space, max_grouping_len):
    tv, sents = _tiny(ignore_space, max_grouping_len)
    _check_properties(tv, sents[:511] + [b"", b"  "], 4)


def test_a_sentence_that_outgrows_the_lds_tier():
    """the arena holds 25 bytes per character before the first node (class, end-list offset, trie code, byte offset, groupable run,
    candidate offset, reachability, lengths: 4 + 4 + 2 + 2 + 2 + 2 + 1 + 8): >= 5000 characters need >= 125 000 bytes, the LDS tier
    is 32 768 (and can be at most 65 536)"""
    tv, sents = _tiny()
    long = b"".join(sents)
    while len(long.decode()) < 5000:
        long += long
    long = long.decode()[:5000].encode()
    assert 25 * 5000 > 65536
    nb = _check_properties(tv, sents[:150] + [long] + sents[150:300], 4)
    assert nb.slab_sentences() >= 1 and tv.tokenize_nbest([long], n=4).slab_sentences() == 1


@pytest.mark.parametrize("n", [0, 17])
def test_refuses_n_outside_1_to_16(n):
    with pytest.raises(V.VibratoError) as e:
        V.Tokenizer(V.SystemDictionaryBuilder.from_readers(_lex(WORDS), _matrix(), CHAR, UNK)).tokenize_nbest(["abc"], n=n)
    assert e.value.code == 1


def test_refuses_a_multi_device_tokenizer():
    with pytest.raises(V.VibratoError) as e:
        V.Tokenizer(V.SystemDictionaryBuilder.from_readers(_lex(WORDS), _matrix(), CHAR, UNK), devices=[0, 0]).tokenize_nbest(["abc"], n=2)
    assert e.value.code == 101
