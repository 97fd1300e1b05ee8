"""Tokenizer.tokenize_marginal (MeCab's -m with -t) on the GPU: against exhaustive enumeration in float64 on the dictionaries of
test_gpu_nbest.py (every character a word, no unknown words: the host-side accessors describe the lattice completely), and by
properties on the synthetic dictionary.

Tolerances (derived: a float64 log-sum-exp step errs by a few ulp of its operands, the errors add over the steps, about
8 * steps * 2^-53 * max|alpha|): against enumeration <= 9 steps and |alpha| <= ~400 give ~1e-12, asserted 1e-9; the properties
(<= 5000 steps, |alpha| <= ~5e4 at T = 500) give ~2e-7, asserted 1e-5."""
import functools
import math

import numpy as np
import pytest

import vibrato_amd as V
from test_gpu_nbest import CHAR, SENTS, UNK, WORDS, _lex, _matrix, _tiny, _wide

pytestmark = pytest.mark.gpu

# strictly between two reference probabilities of the `varied` dictionary at T = 3 (the test asserts that none is within 1e-6)
MIN_PROB = 0.1


def _expected(d, text, T):
    """every path of the lattice, by DFS: (log_z, [(start, end, word_id, prob)] in lattice order, the nodes no path visits left out)"""
    conn = functools.lru_cache(None)(d.conn_cost)
    rows, flat = [], []
    for i in range(len(text)):
        row = []
        for wid, end, left, right, cost in d.common_prefix(text[i:]):
            row.append((len(flat), i + end, left, right, cost))
            flat.append((i, i + end, wid))
        rows.append(row)
    paths = []

    def walk(pos, right, total, seq):
        if pos == len(text):
            paths.append((total + conn(right, 0), seq))
            return
        for q, end, left, r, cost in rows[pos]:
            walk(end, r, total + cost + conn(right, left), seq + (q,))

    if not text:
        return 0.0, []
    walk(0, 0, 0, ())
    assert 0 < len(paths) < 10 ** 5
    c_min = min(c for c, _ in paths)
    weights = [math.exp((c_min - c) / T) for c, _ in paths]
    total = math.fsum(weights)
    per = [[] for _ in flat]
    for w, (_, seq) in zip(weights, paths):
        for q in seq:
            per[q].append(w)
    return -c_min / T + math.log(total), [(s, e, wid, math.fsum(p) / total) for (s, e, wid), p in zip(flat, per) if p and math.fsum(p) > 0]


def _homographs(h):
    return V.SystemDictionaryBuilder.from_readers(_lex([("a", 1 + i % 3, 1 + i % 2, i % 4) for i in range(h)]), _matrix(), CHAR, UNK)


DICTS = {"varied": lambda: V.SystemDictionaryBuilder.from_readers(_lex(WORDS), _matrix(), CHAR, UNK),
         "zero": lambda: V.SystemDictionaryBuilder.from_readers(_lex(WORDS, True), _matrix(True), CHAR, UNK),
         "wide": _wide}
# (id, dictionary, sentences, temperature, min_prob, environment, sentences expected in the slab tier)
CASES = [(f"{k}-T{t}", k, SENTS, t, 0.0, {}, 0) for k in ("varied", "zero") for t in (0.5, 3, 1000)]
CASES += [(f"slab-T{t}", "varied", SENTS, t, 0.0, {"VBT_MARGINAL_LDS_KB": "0"}, len(SENTS) - 1) for t in (0.5, 3, 1000)]
CASES += [(f"wide-T{t}", "wide", SENTS, t, 0.0, {}, 0) for t in (20000, 1e6)]
CASES += [("min_prob", "varied", SENTS, 3, MIN_PROB, {}, 0)]
# h homographs of "a": more predecessors than a row has lanes (h > 16), more than 256, more candidates than a wave has rows -- and in
# the backward sweep the same borders with the roles exchanged; 2 h + h^2 connection costs, more than 32 KiB of them at h = 300
CASES += [(f"h{h}", h, ["aa"], 3, 0.0, {}, 1 if h == 300 else 0) for h in (15, 16, 17, 65, 300)]
# a staging capped at 1 KiB, i.e. at the largest step (h^2 cells, which is what the kernel then stages at most): both sweeps run in
# three blocks of steps and the backward sweep gathers again.  No LDS size admits h = 300 (its largest step alone is 180 000 bytes):
# that one runs in a slab with the capped staging, h = 65 in the LDS tier.
CASES += [(f"blocks-h{h}", h, ["aa"], 3, 0.0, {"VBT_MARGINAL_STAGE_KB": "1"}, 1 if h == 300 else 0) for h in (65, 300)]


@pytest.mark.parametrize("kind,sents,T,min_prob,env,slab", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_against_enumeration(kind, sents, T, min_prob, env, slab, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if "VBT_MARGINAL_STAGE_KB" in env:
        assert 2 * kind + kind * kind > max(kind * kind, 1024 // 2)  # total pairs > the cells staged at once (i16 cells)
    tv = V.Tokenizer(_homographs(kind) if isinstance(kind, int) else DICTS[kind]())
    d, mg = tv.dictionary(), tv.tokenize_marginal(sents, temperature=T, min_prob=min_prob)
    node_off, log_z, nodes = mg.arrays()
    assert len(mg) == len(sents) and node_off[0] == 0 and node_off[-1] == len(nodes) and (nodes["reserved"] == 0).all()
    for s, text in enumerate(sents):
        exp_z, exp = _expected(d, text, T)
        if min_prob:
            assert all(abs(p - min_prob) > 1e-6 for *_, p in exp)
            exp = [e for e in exp if e[3] >= min_prob]
        got = mg.nodes(s)
        assert got.tobytes() == nodes[int(node_off[s]):int(node_off[s + 1])].tobytes()
        assert [(int(g["start_char"]), int(g["end_char"]), int(g["word_idx"])) for g in got] == [e[:3] for e in exp], (text, T)
        assert (got["start_byte"] == got["start_char"]).all() and (got["end_byte"] == got["end_char"]).all()
        dev = max((abs(float(g["prob"]) - e[3]) for g, e in zip(got, exp)), default=0.0)
        print(f"{text!r}: max |prob - ref| = {dev:.3e}, log_z - ref = {mg.log_z(s) - exp_z:.3e}")
        assert dev <= 1e-9, (text, T)
        assert mg.log_z(s) == log_z[s] and abs(log_z[s] - exp_z) <= 1e-9 * max(1.0, abs(exp_z)), (text, T)
    assert mg.slab_sentences() == slab


@pytest.mark.parametrize("ignore_space,max_grouping_len,long", [(False, 0, False), (False, 24, False), (True, 0, False), (True, 24, False), (False, 0, True)])
def test_properties_on_the_synthetic_dictionary(ignore_space, max_grouping_len, long):
    """every path covers every character exactly once (at most once where spaces are skipped), the 1-best's nodes carry at least
    the 1-best's probability, Z holds at least the 1-best's weight; `long`: a 5000-character sentence, which outgrows the LDS tier
    (25 bytes per character before the first node), among 300 short ones"""
    T = 500.0
    tv, sents = _tiny(ignore_space, max_grouping_len)
    sents = sents[:511] + [b"", b"  "]
    if long:
        big = b"".join(sents)
        while len(big.decode()) < 5000:
            big += big
        sents = sents[:150] + [big.decode()[:5000].encode()] + sents[150:300]
    mg, nb, one = tv.tokenize_marginal(sents, temperature=T), tv.tokenize_nbest(sents, n=1), tv.tokenize_batch(sents)
    node_off, log_z, nodes = mg.arrays()
    assert mg.slab_sentences() >= 1 if long else mg.slab_sentences() == 0
    worst = 0.0
    for s, text in enumerate(sents):
        got, n = nodes[int(node_off[s]):int(node_off[s + 1])], len(text.decode())
        cover = np.zeros(n + 1)
        np.add.at(cover, got["start_char"], got["prob"])
        np.add.at(cover, got["end_char"], -got["prob"])
        excess = np.cumsum(cover)[:n] - 1
        if not ignore_space:
            excess = abs(excess)
        worst = max(worst, excess.max(initial=0.0))
        assert (excess <= 1e-5).all(), s
        if nb.num_paths(s) == 0:
            assert len(got) == 0 and log_z[s] == 0
            continue
        c_best = nb.path(s, 0)[0]
        floor = math.exp(-c_best / T - log_z[s]) * (1 - 1e-5)
        if not ignore_space:
            assert log_z[s] >= -c_best / T - 1e-5 * abs(c_best / T), s
        index = {(int(g["start_char"]), int(g["end_char"]), int(g["word_idx"])): float(g["prob"]) for g in got}  # (an unknown word of two lengths: one word_idx)
        for t in one.records(s):
            assert index.get((int(t["start_char"]), int(t["end_char"]), int(t["word_idx"])), 0.0) >= floor, (s, t)
    print(f"worst coverage deviation {worst:.3e}")


@pytest.mark.parametrize("temperature,min_prob,devices,code", [(0, 0, None, 1), (-1, 0, None, 1), (math.nan, 0, None, 1), (math.inf, 0, None, 1),
                                                               (3, -0.1, None, 1), (3, 1.5, None, 1), (3, 0, [0, 0], 101)])
def test_refusals(temperature, min_prob, devices, code):
    with pytest.raises(V.VibratoError) as e:
        V.Tokenizer(DICTS["varied"](), devices=devices).tokenize_marginal(["abc"], temperature=temperature, min_prob=min_prob)
    assert e.value.code == code
