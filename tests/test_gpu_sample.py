"""Tokenizer.tokenize_sample (sample.hip) on the GPU: the contract of include/vibrato_hip.h reproduced exactly by a plain Python
reference over the lattices of tests/pyref.py and the host-side accessors (forward weights in 80-digit decimals, a restatement of
Philox4x32-10, the inverse-CDF walk with exact weights), properties on a long sentence, and the refusals.

A draw is AMBIGUOUS when u lies within 1e-9 of a cumulative boundary of the exact weights; a sample with such a draw is left out of
the comparison, at most 1 in 1000 of a case.  (1e-9 is the bound test_gpu_marginal.py asserts for these lattices: <= 9 steps and
|alpha| <~ 400 give ~1e-12 in alpha, a running sum of <= 301 terms adds ~1e-13.)  For the seeds below the reference alone counts no
ambiguous draw in any case.  Philox: the two restatements (this file's, the kernel's) agree with each other and with the published
known-answer vector for counter 0, key 0."""
import decimal
import functools
import math

import numpy as np
import pytest

import vibrato_amd as V
from test_gpu_lattice_parity import FIELDS, _accessor_lattice, _case, _conn, _lattices, _product
from test_gpu_marginal import DICTS, _homographs
from test_gpu_nbest import SENTS, _tiny
from tests import latref

pytestmark = pytest.mark.gpu
M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    c, k = list(counter), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return c


def reference(lat, conn, T, n_samples, seed, s):
    """(log_z, [(path_cost, records) per sample, None for a sample with an ambiguous draw]) of the sentence with index s"""
    nodes, ends, ctx = lat["nodes"], latref.end_lists(lat), latref._CTX
    if not nodes:  # an empty sentence: no paths; skipped spaces only: paths of no tokens
        return 0.0, [(0, [])] * (n_samples if lat["num_chars"] else 0)
    zero, one, t = decimal.Decimal(0), decimal.Decimal(1), decimal.Decimal(T)
    w = functools.lru_cache(None)(lambda cost: ctx.exp(ctx.divide(decimal.Decimal(-cost), t)))
    right = lambda p: 0 if p == latref.BOS else nodes[p]["right"]  # noqa: E731
    alpha = []
    edges = lambda preds, left: [ctx.multiply(one if p == latref.BOS else alpha[p], w(conn(right(p), left))) for p in preds]  # noqa: E731
    for nd in nodes:
        alpha.append(ctx.multiply(functools.reduce(ctx.add, edges(ends[nd["start_node"]], nd["left"]), zero), w(nd["wcost"])))
    samples = []
    for r in range(n_samples):
        preds, left, path, clear = ends[lat["eos_from"]], 0, [], True
        while preds is not None:
            ps = edges(preds, left)
            total = functools.reduce(ctx.add, ps, zero)
            u = decimal.Decimal(2 * philox4x32_10((s & M32, s >> 32, r, len(path)), (seed & M32, seed >> 32))[0] + 1) / 2 ** 33
            acc, chosen = zero, None
            for j, p in enumerate(ps):
                acc = ctx.add(acc, p)
                clear &= abs(ctx.divide(acc, total) - u) > decimal.Decimal("1e-9")
                if chosen is None and acc > ctx.multiply(u, total):
                    chosen = j
            if preds[chosen] == latref.BOS:
                preds = None
            else:
                path.append(preds[chosen])
                preds, left = ends[nodes[path[-1]]["start_node"]], nodes[path[-1]]["left"]
        total, prev, recs = 0, latref.BOS, []
        for c in reversed(path):
            total += conn(right(prev), nodes[c]["left"]) + nodes[c]["wcost"]
            recs.append(tuple(nodes[c][f] for f in ("start_word", "end", "start_byte", "end_byte")) + ((nodes[c]["lex"] << 30) | nodes[c]["wid"], latref._wrap_i32(total)))
            prev = c
        samples.append((total + conn(right(prev), 0), recs) if clear else None)
    return float(ctx.ln(functools.reduce(ctx.add, edges(ends[lat["eos_from"]], 0), zero))), samples


def check(sm, refs, n_samples):
    """every unambiguous sample record by record and in path_cost, log_z to 1e-9; returns (samples compared, samples left out)"""
    path_off, tok_off, costs, log_z, toks = sm.arrays()
    assert len(sm) == len(refs) and path_off[0] == 0 and path_off[-1] == len(costs) == len(tok_off) - 1 and tok_off[-1] == len(toks)
    done = skipped = 0
    for s, (exp_z, exp) in enumerate(refs):
        p0 = int(path_off[s])
        assert sm.num_paths(s) == int(path_off[s + 1]) - p0 == len(exp), s
        assert sm.log_z(s) == log_z[s] and abs(log_z[s] - exp_z) <= 1e-9 * max(1.0, abs(exp_z)), (s, log_z[s], exp_z)
        for r, e in enumerate(exp):
            if e is None:
                skipped += 1
                continue
            got = toks[int(tok_off[p0 + r]):int(tok_off[p0 + r + 1])]
            assert (int(costs[p0 + r]), [tuple(int(g[f]) for f in FIELDS + ("total_cost",)) for g in got]) == e, (s, r)
            assert sm.path(s, r)[0] == e[0] and sm.path(s, r)[1].tobytes() == got.tobytes()
            done += 1
    assert skipped * 1000 <= done + skipped, (skipped, done)
    return done, skipped


def test_philox_known_answer():
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


# (id, dictionary: a name of DICTS or h homographs of "a", sentences, temperature, n_samples, seed, environment, sentences in the slab tier)
CASES = [(f"{k}-T{t}-n{ns}", k, SENTS, t, ns, 11 + ns, {}, 0) for k in ("varied", "zero") for t in (0.5, 3, 1000) for ns in (1, 4, 5, 64)]
CASES += [(f"wide-T{t}", "wide", SENTS, t, 5, 21, {}, 0) for t in (20000, 1e6)]
# predecessor lists at and across the row width, across a wave, beyond 256; h = 300 outgrows every LDS size
CASES += [(f"h{h}", h, ["aa"], 3, 64 if h == 17 else 5, 31, {}, 1 if h == 300 else 0) for h in (15, 16, 17, 65, 300)]
CASES += [("slab", "varied", SENTS, 3, 5, 41, {"VBT_MARGINAL_LDS_KB": "0"}, len(SENTS) - 1)]
CASES += [(f"blocks-h{h}", h, ["aa"], 3, 5, 51, {"VBT_MARGINAL_STAGE_KB": "1"}, 1 if h == 300 else 0) for h in (65, 300)]  # the walks cross staging blocks


@pytest.mark.parametrize("kind,sents,T,n_samples,seed,env,slab", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_reproduces_the_contract(kind, sents, T, n_samples, seed, env, slab, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tv = V.Tokenizer(_homographs(kind) if isinstance(kind, int) else DICTS[kind]())
    d = tv.dictionary()
    conn = functools.lru_cache(None)(d.conn_cost)
    refs = [reference(_accessor_lattice(d, text), conn, T, n_samples, seed, s) for s, text in enumerate(sents)]
    sm = tv.tokenize_sample(sents, temperature=T, n_samples=n_samples, seed=seed)
    print("compared %d samples, left out %d" % check(sm, refs, n_samples))
    assert sm.slab_sentences() == slab


@pytest.mark.parametrize("ignore_space,mgl", [(False, 0), (True, 1), (True, 3)])
@pytest.mark.parametrize("dict_seed", [3, 5])
def test_reproduces_the_contract_on_the_tie_heavy_dictionaries(dict_seed, ignore_space, mgl):
    """unknown words, grouping, skipped spaces, a user lexicon, multi-byte text (test_gpu_lattice_parity.py's inputs)"""
    d, sents = _case(dict_seed)
    lats = _lattices(dict_seed, ignore_space, mgl)
    refs = [reference(lat, _conn(d), 3, 4, 7, s) for s, lat in enumerate(lats)]
    sm = _product(d, ignore_space, mgl).tokenize_sample(list(sents), temperature=3, n_samples=4, seed=7)
    print("compared %d samples, left out %d" % check(sm, refs, 4))


def test_determinism_and_the_renumbered_image():
    """the same call twice: the same bytes; the sentences reversed: each sentence's samples are those of its NEW index; after the
    connection ids were renumbered: the same bytes again"""
    d, sents = _case(5)
    sents, lats = list(sents), _lattices(5, False, 0)
    for repeat in (1, 8, 64):  # a tokenizer calibrates once: a larger sample needs a fresh one
        tv = _product(d, False, 0)
        first, again = [tv.tokenize_sample(sents, temperature=3, n_samples=5, seed=9).arrays() for _ in range(2)]
        back = tv.tokenize_sample(sents[::-1], temperature=3, n_samples=5, seed=9)
        if tv.calibrate(sentences=sents * repeat)["epoch"] == 1:
            break
    assert tv.connid_reorder_info()["epoch"] == 1
    renumbered = tv.tokenize_sample(sents, temperature=3, n_samples=5, seed=9)
    for a, b, c in zip(first, again, renumbered.arrays()):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    check(renumbered, [reference(lat, _conn(d), 3, 5, 9, s) for s, lat in enumerate(lats)], 5)
    check(back, [reference(lat, _conn(d), 3, 5, 9, s) for s, lat in enumerate(lats[::-1])], 5)


@pytest.mark.parametrize("ignore_space,max_grouping_len", [(False, 0), (True, 24)])
def test_properties_with_a_long_sentence(ignore_space, max_grouping_len):
    """a 5000-character sentence (the slab tier) among 300 short ones at T = 500: 5000 steps put alpha's error near 2e-7, so no exact
    reproduction here; every sampled path tiles its sentence with nodes the marginals report, at the cost the host recomputes"""
    T, ns = 500.0, 4
    tv, sents = _tiny(ignore_space, max_grouping_len)
    big = b"".join(sents)
    while len(big.decode()) < 5000:
        big += big
    sents = sents[:150] + [big.decode()[:5000].encode()] + sents[150:300]
    d, sm, mg = tv.dictionary(), tv.tokenize_sample(sents, temperature=T, n_samples=ns, seed=5), tv.tokenize_marginal(sents, temperature=T)
    path_off, tok_off, costs, log_z, toks = sm.arrays()
    node_off, mg_z, nodes = mg.arrays()
    assert sm.slab_sentences() >= 1 and tv.tokenize_sample([sents[150]], temperature=T, n_samples=ns).slab_sentences() == 1
    param, conn = {}, {}
    for s, text in enumerate(sents):
        assert sm.num_paths(s) == (ns if text else 0) and abs(log_z[s] - mg_z[s]) <= 1e-5 * max(1.0, abs(mg_z[s])), s
        reported = {tuple(int(g[f]) for f in FIELDS) for g in nodes[int(node_off[s]):int(node_off[s + 1])]}
        for p in range(int(path_off[s]), int(path_off[s + 1])):
            right, total, at = 0, 0, 0
            for t in toks[int(tok_off[p]):int(tok_off[p + 1])]:
                w = int(t["word_idx"])
                left, r, wc = param.setdefault(w, d.word_param(w >> 30, w & 0x3FFFFFFF))
                total += wc + conn.setdefault((right, left), d.conn_cost(right, left))
                assert tuple(int(t[f]) for f in FIELDS) in reported and latref._wrap_i32(total) == t["total_cost"], (s, p)
                assert t["start_byte"] == at or (ignore_space and text[at:t["start_byte"]].decode().isspace()), (s, p)  # contiguous
                right, at = r, int(t["end_byte"])
            assert at == len(text) or (ignore_space and text[at:].decode().isspace()), (s, p)
            assert total + conn.setdefault((right, 0), d.conn_cost(right, 0)) == costs[p], (s, p)


@pytest.mark.parametrize("temperature,n_samples,devices,code", [(0, 1, None, 1), (-1, 1, None, 1), (math.nan, 1, None, 1), (math.inf, 1, None, 1),
                                                                 (3, 0, None, 1), (3, 65, None, 1), (3, 1, [0, 0], 101)])
def test_refusals(temperature, n_samples, devices, code):
    with pytest.raises(V.VibratoError) as e:
        V.Tokenizer(DICTS["varied"](), devices=devices).tokenize_sample(["abc"], temperature=temperature, n_samples=n_samples)
    assert e.value.code == code
