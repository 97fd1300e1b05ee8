"""tests/latref.py (the N-best and marginal reference of test_gpu_lattice_parity.py) anchored without a GPU: on the lattices of
pyref.PyTokenizer.lattice() -- the random tie-heavy dictionaries of test_oracle_vs_python_restatement.py, with unknown words, grouping,
skipped spaces, a user lexicon and multi-byte text -- kbest(1) is PyTokenizer.tokenize() record by record, and where a sentence has few
enough paths kbest(16) and marginals() equal the exhaustive enumeration of its paths."""
import functools
import math
import random

import pytest

from tests import latref, pyref
from tests.test_oracle_vs_python_restatement import make_dictionary, make_sentence

EDGE = ["", " ", "  あ  ", "あ ", " a1 ", "𠮷", "1111", "ああああああああ"]
CONFIGS = [(ignore_space, mgl) for ignore_space in (False, True) for mgl in (0, 1, 3)]
# Enumerated: the sentences with at most this many paths (counted by latref.count_paths, an integer sweep).  enumerate_paths itself
# asserts fewer than 10^5; 4000 keeps the 12 x 6 x 68 sentences of this module within seconds and still leaves 78 .. 122 sentences
# with more than 16 paths per seed (the test asserts at least 20).
ENUM_PATHS = 4000


@functools.lru_cache(maxsize=None)
def _case(seed):
    rng = random.Random(20260925 + seed)
    d = make_dictionary(rng)
    return d, [make_sentence(rng) for _ in range(60)] + EDGE


def _tokenizer(d, ignore_space, mgl):
    return pyref.PyTokenizer(d["lex"], d["n_ids"], d["n_ids"], d["matrix"], d["char_def"], d["unk"], user_csv=d["user"],
                             ignore_space=ignore_space, max_grouping_len=mgl)


def _conn(d):
    return lambda right, left: d["matrix"][left * d["n_ids"] + right]


def _records(tokens):
    return [(t["start_char"], t["end_char"], t["start_byte"], t["end_byte"], t["word_idx"], t["total_cost"]) for t in tokens]


@pytest.mark.parametrize("seed", range(12))
def test_the_lattice_and_its_best_path_are_tokenize(seed):
    d, sentences = _case(seed)
    for ignore_space, mgl in CONFIGS:
        py, other = _tokenizer(d, ignore_space, mgl), _tokenizer(d, ignore_space, mgl)
        for s in sentences:
            exp = other.tokenize(s)
            before = dict(py.counters)
            lat = py.lattice(s)
            assert py.counters == before  # lattice() counts nothing
            assert py.tokenize(s) == exp
            starts = [nd["start_word"] for nd in lat["nodes"]]
            assert lat["num_chars"] == len(s) and starts == sorted(starts)  # lattice order: by start position, then insertion
            for nd in lat["nodes"]:
                assert (nd["start_byte"], nd["end_byte"]) == (len(s[:nd["start_word"]].encode()), len(s[:nd["end"]].encode()))
            best = latref.kbest(lat, _conn(d), 1)
            if s == "":
                assert best == [] and exp == []
                continue
            assert len(best) == 1 and best[0][1] == _records(exp), (seed, ignore_space, mgl, s)
            last = lat["nodes"][_node_of(lat, exp[-1])]["right"] if exp else 0
            assert best[0][0] == (exp[-1]["total_cost"] if exp else 0) + _conn(d)(last, 0)
        assert py.counters == other.counters


def _node_of(lat, t):
    """index of the lattice node a token record names (start, end and word identify a node)"""
    hits = [i for i, nd in enumerate(lat["nodes"]) if (nd["start_word"], nd["end"], (nd["lex"] << 30) | nd["wid"]) == (t["start_char"], t["end_char"], t["word_idx"])]
    assert len(hits) == 1
    return hits[0]


@pytest.mark.parametrize("seed", range(12))
def test_kbest_and_marginals_against_enumeration(seed):
    d, sentences = _case(seed)
    conn = _conn(d)
    enumerated = beyond_16 = dead_ends = 0
    worst = 0.0
    for ignore_space, mgl in CONFIGS:
        py = _tokenizer(d, ignore_space, mgl)
        for s in sentences:
            lat = py.lattice(s)
            if latref.count_paths(lat) > ENUM_PATHS:
                continue
            paths = latref.enumerate_paths(lat, conn)
            assert len(paths) == latref.count_paths(lat) < 10 ** 5
            nodes = lat["nodes"]
            enumerated += 1
            beyond_16 += len(paths) > 16
            # the contract's key: cost, then from EOS backwards the node inserted later first (one end list: the larger slot)
            ordered = sorted(paths, key=lambda p: (p[0], [-nodes[c]["slot"] for c in reversed(p[1])]))
            exp = [(cost, [(nodes[c]["start_word"], nodes[c]["end"], nodes[c]["start_byte"], nodes[c]["end_byte"],
                            (nodes[c]["lex"] << 30) | nodes[c]["wid"], t) for c, t in zip(seq, totals)]) for cost, seq, totals in ordered[:16]]
            assert latref.kbest(lat, conn, 16) == exp, (seed, ignore_space, mgl, s)
            for T in (0.5, 3.0):
                m = latref.marginals(lat, conn, T)
                if not nodes:
                    assert m["log_z"] == 0 and m["prob"] == []
                    continue
                c_min = min(c for c, _, _ in paths)  # (the construction of test_gpu_marginal.py's _expected)
                weights = [math.exp((c_min - c) / T) for c, _, _ in paths]
                total = math.fsum(weights)
                per = [[] for _ in nodes]
                for wgt, (_, seq, _) in zip(weights, paths):
                    for c in seq:
                        per[c].append(wgt)
                exp_z = -c_min / T + math.log(total)
                assert abs(float(m["log_z"]) - exp_z) <= 1e-12 * max(1.0, abs(exp_z)), (seed, ignore_space, mgl, s, T)
                for c, p in enumerate(per):
                    dev = abs(float(m["prob"][c]) - math.fsum(p) / total)
                    worst = max(worst, dev)
                    assert dev <= 1e-12, (seed, ignore_space, mgl, s, T, c)
                    assert (m["prob"][c] == 0) == (not p)
                dead_ends += sum(not p for p in per)
                assert m["steps"] == len({nodes[c]["start_word"] for c in range(len(nodes))}) + 1 and m["max_abs_alpha"] >= abs(exp_z) * (1 - 1e-9)
    print(f"seed {seed}: {enumerated} sentences enumerated, {beyond_16} with more than 16 paths, {dead_ends} dead-end nodes, worst |prob - enumeration| = {worst:.2e}")
    assert enumerated >= 6 * len(EDGE) and beyond_16 >= 20


def test_wrapping_and_exact_sums():
    """kbest wraps entry by entry and orders by the wrapped values; marginals sums exact integers"""
    big = 2 ** 30
    lat = {"num_chars": 3, "eos_from": 3, "nodes": [
        {"start_node": p, "start_word": p, "end": p + 1, "start_byte": p, "end_byte": p + 1, "lex": 0, "wid": 2 * p + h, "left": h, "right": h,
         "wcost": 0, "slot": h} for p in range(3) for h in (0, 1)]}
    conn = lambda right, left: big if right == left == 1 else 0  # noqa: E731
    paths = latref.kbest(lat, conn, 16)
    assert len(paths) == 8
    assert paths[0][0] == latref._wrap_i32(2 * big) == -2 ** 31  # 1 -> 1 -> 1: two steps of 2^30 wrap and come first
    assert [r[5] for r in paths[0][1]] == [0, big, -2 ** 31]
    m = latref.marginals(lat, conn, float(big))
    z = 5 + 2 * math.exp(-1) + math.exp(-2)  # exact sums: 5 paths of cost 0, 2 of 2^30, 1 of 2^31
    assert abs(float(m["log_z"]) - math.log(z)) <= 1e-15 * 8
    assert abs(float(m["prob"][5]) - (2 + math.exp(-1) + math.exp(-2)) / z) <= 1e-15
