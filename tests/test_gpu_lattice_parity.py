"""Tokenizer.tokenize_nbest (nbest.hip) and Tokenizer.tokenize_marginal (marginal.hip) against tests/latref.py on the lattices of
tests/pyref.py: the random tie-heavy dictionaries of test_oracle_vs_python_restatement.py -- unknown words of every invoke / group /
length combination, grouping limits, skipped spaces (start_node != start_word, dead ends, "input ends with spaces"), a user lexicon,
2-, 3- and 4-byte characters -- where both kernels restate the generator phases, and which the exact references of test_gpu_nbest.py
and test_gpu_marginal.py (ASCII, every character a word) do not reach.  tests/test_lattice_reference.py anchors the reference.

Marginal tolerance (the derivation of test_gpu_marginal.py's docstring: a float64 log-sum-exp step errs by a few ulp of its operands
and the errors add over the steps): bound = 8 * steps * 2^-53 * max|alpha|, per sentence, from the REFERENCE's step count and largest
|log forward weight|; asserted at 100 x bound with a floor of 1e-12, absolutely on prob and scaled by max(1, |log_z|) on log_z.  Every
test prints the worst error / bound it saw."""
import decimal
import functools
import random

import numpy as np
import pytest

import vibrato_amd as V
from test_gpu_marginal import _homographs
from test_gpu_nbest import CHAR, SENTS, UNK, WORDS, _lex, _wide
from tests import latref, pyref
from tests.test_oracle_vs_python_restatement import ALPHA, HIRA, KATA, NUM, OTHER, make_dictionary, make_sentence

pytestmark = pytest.mark.gpu

# Six of the twelve dictionaries of test_lattice_reference.py, chosen on the reference alone: every connection matrix is asymmetric;
# 7 has no user lexicon, the user entries of the other five match in the sentences (25 .. 145 user nodes); 3 and 11 have dead-end
# nodes under ignore_space; 5 and 10 have five connection ids, 8 has two.  test_the_inputs_reach_what_they_are_chosen_for holds this.
SEEDS = (3, 5, 7, 8, 10, 11)
CONFIGS = ((False, 0), (True, 1), (True, 3))  # (ignore_space, max_grouping_len)
EDGE = ["", " ", "  あ  ", "あ ", " a1 ", "𠮷", "1111", "ああああああああ"]
FIELDS = ("start_char", "end_char", "start_byte", "end_byte", "word_idx")
TINY = decimal.Decimal("1e-290")  # (the smallest normal float64 is 2.2e-308)
SENTENCE_ALPHABET = HIRA * 3 + KATA * 2 + ALPHA * 2 + NUM + "   " + OTHER  # (make_sentence's)


@functools.lru_cache(maxsize=None)
def _case(seed):
    rng = random.Random(20260925 + seed)
    d = make_dictionary(rng)
    return d, [make_sentence(rng) for _ in range(60)] + EDGE


def _conn(d):
    return lambda right, left: d["matrix"][left * d["n_ids"] + right]


def _product(d, ignore_space, mgl):
    dv = V.SystemDictionaryBuilder.from_readers(d["lex"], d["matrix_def"], d["char_def"], d["unk"])
    if d["user"] is not None:
        dv.reset_user_lexicon_from_reader(d["user"])
    return V.Tokenizer(dv).ignore_space(ignore_space).max_grouping_len(mgl)


@functools.lru_cache(maxsize=None)
def _lattices(seed, ignore_space, mgl):
    """the reference lattices of the dictionary's sentences: built once, left unchanged"""
    d, sents = _case(seed)
    py = pyref.PyTokenizer(d["lex"], d["n_ids"], d["n_ids"], d["matrix"], d["char_def"], d["unk"], user_csv=d["user"],
                           ignore_space=ignore_space, max_grouping_len=mgl)
    return tuple(py.lattice(s) for s in sents)


def _check_nbest(nb, lats, conn, n):
    path_off, tok_off, costs, toks = nb.arrays()
    assert len(nb) == len(lats) and path_off[0] == 0 and path_off[-1] == len(costs) == len(tok_off) - 1 and tok_off[-1] == len(toks)
    for s, lat in enumerate(lats):
        exp = latref.kbest(lat, conn, n)
        p0 = int(path_off[s])
        assert nb.num_paths(s) == int(path_off[s + 1]) - p0 == len(exp), (s, n)
        for r, (cost, recs) in enumerate(exp):
            got = toks[int(tok_off[p0 + r]):int(tok_off[p0 + r + 1])]
            assert int(costs[p0 + r]) == cost, (s, n, r)
            assert [tuple(int(t[f]) for f in FIELDS + ("total_cost",)) for t in got] == recs, (s, n, r)
        if lat["num_chars"] == 0:
            assert exp == []  # an empty sentence: no path
        elif not lat["nodes"]:
            assert [len(recs) for _, recs in exp] == [0]  # skipped spaces only: one path of no tokens


class Worst:
    """the worst error / bound of a test, over the sentences whose tolerance is 100 x bound, and the worst error under the 1e-12 floor"""

    def __init__(self):
        self.ratio, self.under_floor = 0.0, 0.0

    def add(self, err, bound):
        if 100 * bound >= 1e-12:
            self.ratio = max(self.ratio, err / bound)
        else:
            self.under_floor = max(self.under_floor, err)

    def __str__(self):
        return f"worst error / bound = {self.ratio:.3f}; worst error where the 1e-12 floor applies = {self.under_floor:.3e}"


def _check_marginal(mg, lats, conn, T, worst, min_prob=0.0, refs=None):
    node_off, log_z, nodes = mg.arrays()
    assert len(mg) == len(lats) and node_off[0] == 0 and node_off[-1] == len(nodes) and (np.diff(node_off.astype(np.int64)) >= 0).all()
    assert (nodes["reserved"] == 0).all()
    for s, lat in enumerate(lats):
        ref = refs[s] if refs is not None else latref.marginals(lat, conn, T)
        bound = 8 * ref["steps"] * 2.0 ** -53 * ref["max_abs_alpha"]
        tol = max(100 * bound, 1e-12)
        # "positive in float64": the inputs keep clear of the border, so that the reference decides membership
        assert all(p == 0 or p > TINY for p in ref["prob"]), s
        if min_prob:
            assert all(abs(float(p) - min_prob) > 1e-6 for p in ref["prob"]), s
        exp = [(tuple(nd[k] for k in ("start_word", "end", "start_byte", "end_byte")) + ((nd["lex"] << 30) | nd["wid"],), float(p))
               for nd, p in zip(lat["nodes"], ref["prob"]) if p > 0 and p >= min_prob]
        got = nodes[int(node_off[s]):int(node_off[s + 1])]
        assert len(got) == len(exp), (s, T, len(got), len(exp))  # exactly the reference count
        assert [tuple(int(g[f]) for f in FIELDS) for g in got] == [e[0] for e in exp], (s, T)
        err = max((abs(float(g["prob"]) - e[1]) for g, e in zip(got, exp)), default=0.0)
        err_z = abs(float(log_z[s]) - float(ref["log_z"])) / max(1.0, abs(float(ref["log_z"])))
        worst.add(max(err, err_z), bound)
        assert err <= tol, (s, T, err, tol)
        assert err_z <= tol, (s, T, err_z, tol)
        if not lat["nodes"]:
            assert log_z[s] == 0 and len(got) == 0  # an empty sentence, or skipped spaces only


def test_the_inputs_reach_what_they_are_chosen_for():
    dead_ends = 0
    for seed in SEEDS:
        d, sents = _case(seed)
        n, m = d["n_ids"], d["matrix"]
        assert any(m[a * n + b] != m[b * n + a] for a in range(n) for b in range(a)), seed  # swapped ids would show
        for ignore_space, mgl in CONFIGS:
            lats = _lattices(seed, ignore_space, mgl)
            nodes = [nd for lat in lats for nd in lat["nodes"]]
            assert {nd["lex"] for nd in nodes} == ({0, 1, 2} if d["user"] is not None else {0, 2}), seed
            assert any(nd["end_byte"] - nd["start_byte"] > nd["end"] - nd["start_word"] for nd in nodes)  # multi-byte text
            assert any(nd["start_byte"] == 4 and nd["start_word"] == 1 for nd in nodes)  # behind a 4-byte character
            if ignore_space:
                assert any(nd["start_node"] != nd["start_word"] for nd in nodes), seed  # a step behind skipped spaces
                assert any(lat["eos_from"] != lat["num_chars"] for lat in lats), seed  # "input ends with spaces"
                dead_ends += sum(p == 0 for lat in lats for p in latref.marginals(lat, _conn(d), 3)["prob"])
    assert dead_ends > 0


# ---- (a) N-best, exact


@pytest.mark.parametrize("n", [1, 4, 16])
@pytest.mark.parametrize("ignore_space,mgl", CONFIGS)
@pytest.mark.parametrize("seed", SEEDS)
def test_nbest_equals_the_lattice_reference(seed, ignore_space, mgl, n):
    d, sents = _case(seed)
    tv, lats = _product(d, ignore_space, mgl), _lattices(seed, ignore_space, mgl)
    nb = tv.tokenize_nbest(list(sents), n=n)
    _check_nbest(nb, lats, _conn(d), n)


# ---- (b) marginals


@pytest.mark.parametrize("T", [0.5, 3, 1000])
@pytest.mark.parametrize("ignore_space,mgl", CONFIGS)
@pytest.mark.parametrize("seed", SEEDS)
def test_marginals_equal_the_lattice_reference(seed, ignore_space, mgl, T):
    d, sents = _case(seed)
    tv, lats = _product(d, ignore_space, mgl), _lattices(seed, ignore_space, mgl)
    worst = Worst()
    mg = tv.tokenize_marginal(list(sents), temperature=T)
    _check_marginal(mg, lats, _conn(d), T, worst)
    print(f"seed {seed} ignore_space {ignore_space} max_grouping_len {mgl} T {T}: {worst}")


# ---- (c) the slab tier and a long sentence


@functools.lru_cache(maxsize=None)
def _long_case():
    """seed 3 under (ignore_space, max_grouping_len 3): 20 short sentences around two of 400 and 1200 characters"""
    d, sents = _case(3)
    rng = random.Random(20261126)
    long = ["".join(rng.choice(SENTENCE_ALPHABET) for _ in range(k)) for k in (400, 1200)]
    sents = sents[:10] + long[:1] + sents[10:16] + EDGE[1:4] + long[1:] + sents[16:17]
    assert len(sents) == 22
    py = pyref.PyTokenizer(d["lex"], d["n_ids"], d["n_ids"], d["matrix"], d["char_def"], d["unk"], user_csv=d["user"], ignore_space=True, max_grouping_len=3)
    lats = tuple(py.lattice(s) for s in sents)
    for k in (10, 20):  # 25 bytes per character + about 30 per node: more than the 32 KiB of the LDS tier
        assert 25 * lats[k]["num_chars"] + 30 * len(lats[k]["nodes"]) > 32768
    return d, sents, lats


def test_long_sentences_in_the_slab_tier():
    d, sents, lats = _long_case()
    tv, worst = _product(d, True, 3), Worst()
    nb = tv.tokenize_nbest(sents, n=4)
    _check_nbest(nb, lats, _conn(d), 4)
    mg = tv.tokenize_marginal(sents, temperature=3)
    _check_marginal(mg, lats, _conn(d), 3, worst)
    in_slab = {k: (tv.tokenize_nbest([sents[k]], n=4).slab_sentences(), tv.tokenize_marginal([sents[k]], temperature=3).slab_sentences()) for k in (10, 20)}
    print(f"slab sentences: n-best {nb.slab_sentences()}, marginal {mg.slab_sentences()}; alone (n-best, marginal): "
          f"400 characters {in_slab[10]}, 1200 characters {in_slab[20]}; {worst}")
    assert nb.slab_sentences() >= 1 and mg.slab_sentences() >= 1


def test_short_sentences_with_every_lattice_in_global_memory(monkeypatch):
    monkeypatch.setenv("VBT_NBEST_LDS_KB", "0")
    monkeypatch.setenv("VBT_MARGINAL_LDS_KB", "0")
    d, sents, lats = _long_case()
    short = [k for k in range(len(sents)) if k not in (10, 20)]
    sents, lats = [sents[k] for k in short], [lats[k] for k in short]
    tv, worst = _product(d, True, 3), Worst()
    nb = tv.tokenize_nbest(sents, n=4)
    _check_nbest(nb, lats, _conn(d), 4)
    mg = tv.tokenize_marginal(sents, temperature=3)
    _check_marginal(mg, lats, _conn(d), 3, worst)
    walked = sum(1 for lat in lats if lat["num_chars"])  # an empty sentence never asks for an arena
    assert nb.slab_sentences() == walked and mg.slab_sentences() == walked
    print(f"{walked} sentences in slabs: {worst}")


# ---- (d) a calibrated image


def test_after_the_connection_ids_were_renumbered():
    """both kernels read the image's matrix and word parameters: results must not depend on the image's numbering"""
    d, sents = _case(5)
    sents = list(sents)
    lats = _lattices(5, False, 0)
    for repeat in (1, 8, 64):  # a tokenizer calibrates once: a larger sample needs a fresh one
        tv = _product(d, False, 0)
        assert tv.connid_reorder_info()["epoch"] == 0
        nb0, mg0 = tv.tokenize_nbest(sents, n=4), tv.tokenize_marginal(sents, temperature=3)
        info = tv.calibrate(sentences=sents * repeat)
        if info["epoch"] == 1:
            break
    assert info["state"] == "done" and info["epoch"] == 1 and info["moved_left"] + info["moved_right"] > 0, info
    nb1, mg1 = tv.tokenize_nbest(sents, n=4), tv.tokenize_marginal(sents, temperature=3)
    assert tv.connid_reorder_info()["epoch"] == 1
    _check_nbest(nb0, lats, _conn(d), 4)
    for a, b in zip(nb0.arrays(), nb1.arrays()):
        assert a.tobytes() == b.tobytes()
    worst = Worst()
    _check_marginal(mg0, lats, _conn(d), 3, worst)
    _check_marginal(mg1, lats, _conn(d), 3, worst)
    (off0, _, nodes0), (off1, _, nodes1) = mg0.arrays(), mg1.arrays()
    assert off0.tobytes() == off1.tobytes() and all(nodes0[f].tobytes() == nodes1[f].tobytes() for f in FIELDS)
    print(f"sample x {repeat}: {info}; {worst}")


# ---- (e) sentences that find the node staging full next to sentences that do not


def _accessor_lattice(d, text):
    """the lattice of an ASCII sentence on a dictionary where every character is a word and nothing else matches (no unknown
    words, no user lexicon), from the host-side accessors -- as _expected of test_gpu_marginal.py builds it"""
    nodes, filled = [], [0] * (len(text) + 1)
    for i in range(len(text)):
        for wid, end, left, right, cost in d.common_prefix(text[i:]):
            nodes.append({"start_node": i, "start_word": i, "end": i + end, "start_byte": i, "end_byte": i + end, "lex": 0, "wid": wid,
                          "left": left, "right": right, "wcost": cost, "slot": filled[i + end]})
            filled[i + end] += 1
    return {"num_chars": len(text), "nodes": nodes, "eos_from": len(text)}


# a workspace for up to 64 sentences and 4096 bytes (the capacities a small batch is rounded up to) starts with a staging of 4 records
# per byte + 64 per sentence
FIRST_STAGING = 4 * 4096 + 64 * 64


@pytest.mark.parametrize("h,sents", [(65, ["a", "aa", "", "aaa", "a"]),
                                     (17, ["a", "a" * 400, "", "a" * 300, "aa", "a" * 350, "a" * 200, "a"])], ids=["h65-455-nodes", "h17-overflow"])
def test_a_batch_of_which_some_sentences_find_the_staging_full(h, sents):
    """h homographs of "a": h nodes per character.  The first batch stays within the first staging of a small batch; the second
    asks for more than it holds while every sentence alone, and all but the largest together, fit: whichever wave takes its range
    first, some sentences are written in the first run and some file themselves for the second -- which has to keep what was
    written and use the ranges already taken."""
    total = h * sum(len(s) for s in sents)
    if h == 17:
        assert total > FIRST_STAGING > h * max(len(s) for s in sents) and total - h * max(len(s) for s in sents) < FIRST_STAGING
    tv = V.Tokenizer(_homographs(h))
    d, worst = tv.dictionary(), Worst()
    lats = [_accessor_lattice(d, s) for s in sents]
    assert sum(len(lat["nodes"]) for lat in lats) == total
    conn = functools.lru_cache(None)(d.conn_cost)
    for _ in range(2):  # the second call finds the staging already enlarged
        mg = tv.tokenize_marginal(sents, temperature=3)
        _check_marginal(mg, lats, conn, 3, worst)
        node_off = mg.arrays()[0]
        assert np.diff(node_off.astype(np.int64)).tolist() == [len(lat["nodes"]) for lat in lats] and node_off[-1] == total
    print(f"{total} nodes against a first staging of {FIRST_STAGING}: {worst}")


# ---- (f) exact sums beyond i32


def _huge():
    """_wide() of test_gpu_nbest.py with connection costs of -1.2e9 .. 1.2e9: the costs of three steps leave i32"""
    ids = "".join(f"{i}\tF{i}\n" for i in (1, 2, 3))
    cost = "".join(f"F{r}/F{l}\t{(r * 7 + l * 3) % 5 * 600000000 - 1200000000}\n" for r in (1, 2, 3) for l in (1, 2, 3))
    return V.SystemDictionaryBuilder.from_readers_with_bigram_info(_lex(WORDS), ids, ids, cost, CHAR, UNK)


def test_path_costs_beyond_i32_are_summed_exactly():
    tv = V.Tokenizer(_huge())
    d, worst = tv.dictionary(), Worst()
    conn = functools.lru_cache(None)(d.conn_cost)
    assert {abs(conn(r, l)) for r in (1, 2, 3) for l in (1, 2, 3)} == {0, 600000000, 1200000000}
    lats = [_accessor_lattice(d, s) for s in SENTS]
    costs = [c for lat in lats for c, _, _ in latref.enumerate_paths(lat, conn)]
    assert min(costs) < -2 ** 31 and max(costs) >= 2 ** 31  # no i32 holds them
    _check_marginal(tv.tokenize_marginal(SENTS, temperature=1e9), lats, conn, 1e9, worst)
    print(f"path costs {min(costs)} .. {max(costs)}: {worst}")


# ---- (g) min_prob, and "positive in float64"


def test_min_prob_keeps_exactly_the_nodes_at_or_above_it():
    """0.25 lies at least 1e-6 from every reference probability of these sentences (_check_marginal asserts it)"""
    d, sents = _case(3)
    tv, lats = _product(d, True, 1), _lattices(3, True, 1)
    worst = Worst()
    mg = tv.tokenize_marginal(list(sents), temperature=3, min_prob=0.25)
    _check_marginal(mg, lats, _conn(d), 3, worst, min_prob=0.25)
    kept, positive = len(mg.arrays()[2]), sum(p > 0 for lat in lats for p in latref.marginals(lat, _conn(d), 3)["prob"])
    assert 0 < kept < positive
    print(f"{kept} of {positive} nodes kept: {worst}")


def test_a_probability_that_is_zero_in_float64_is_not_reported():
    """the `wide` dictionary at T = 100: 30 nodes of SENTS have a probability below 1e-400 (the largest 5e-435: exp of it is 0 in
    float64), 14 one above 1e-290 (the smallest 0.495), none lies between"""
    tv = V.Tokenizer(_wide())
    d, worst = tv.dictionary(), Worst()
    conn = functools.lru_cache(None)(d.conn_cost)
    lats = [_accessor_lattice(d, s) for s in SENTS]
    refs = [latref.marginals(lat, conn, 100) for lat in lats]
    probs = [p for ref in refs for p in ref["prob"]]
    low, high = [p for p in probs if p < decimal.Decimal("1e-400")], [p for p in probs if p > TINY]
    assert all(p > 0 for p in probs) and len(low) + len(high) == len(probs) and len(low) >= 10 and len(high) >= 10
    # to the kernel's float64 the first group is 0: the reference with those set to 0 is what it must report
    refs = [dict(ref, prob=[p if p > TINY else 0 for p in ref["prob"]]) for ref in refs]
    mg = tv.tokenize_marginal(SENTS, temperature=100)
    _check_marginal(mg, lats, conn, 100, worst, refs=refs)
    assert len(mg.arrays()[2]) == len(high)
    print(f"{len(low)} nodes below 1e-400 absent, {len(high)} above 1e-290 present: {worst}")
