"""bench.py's own plumbing: what --dump-outputs writes (every sentence, or a fixed seeded sample of a larger output) and what a
plain run -- no --full -- does and prints."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("start_char", "end_char", "start_byte", "end_byte", "word_idx", "total_cost")
N_SENT = 3000


@pytest.fixture(scope="module")
def bench():
    before = os.environ.get("GPU_MAX_HW_QUEUES")
    import bench as b  # (sets a default for the HIP runtime's queues on import: of no concern to this process)
    if before is None:
        os.environ.pop("GPU_MAX_HW_QUEUES", None)
    return b


@pytest.fixture(scope="module")
def oracle_batch():
    """(tokens in sentence order as [T, 6] float64, exclusive token offsets [n + 1]) of the corpus `bench.py --dict small --sentences
    N_SENT` draws, from the CPU oracle."""
    from oracle import oracle as ora
    from tools import synth
    sd = synth.SynthDict("small")
    d = ora.Dictionary.from_sources_binmatrix(sd.lex, sd.matrix, sd.num_right, sd.num_left, sd.char_def, sd.unk)
    text, offs = sd.sentences(N_SENT, "lognormal_40", space_p=0.0, seed=synth.SEED)
    toks, ends = ora.Tokenizer(d).new_worker().tokenize_batch(text, offs)
    rows = np.stack([toks[f].astype(np.float64) for f in FIELDS], axis=1)
    rows.setflags(write=False)
    return toks, rows, np.asarray(ends, dtype=np.int64)


def scattered_parts(toks, ends, cuts, seed):
    """The oracle's records as the device would leave them: per shard (sentences [cuts[i], cuts[i + 1])), token ranges handed out in
    a random order of the shard's sentences."""
    rng = np.random.default_rng(seed)
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        cnt = np.diff(ends[lo:hi + 1]).astype(np.uint32)
        off = np.zeros(hi - lo, dtype=np.uint32)
        out = np.zeros(int(cnt.sum()), dtype=toks.dtype)
        at = 0
        for s in rng.permutation(hi - lo):
            off[s] = at
            out[at:at + cnt[s]] = toks[ends[lo + s]:ends[lo + s + 1]]
            at += int(cnt[s])
        parts.append((off, cnt, out))
    return parts


def load(d):
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert sorted(got) == ["sentences", "tok_cnt", "tokens"]
    assert all(a.dtype == np.float64 for a in got.values())
    return got


def test_dump_outputs_writes_every_sentence_in_sentence_order(bench, oracle_batch, tmp_path):
    toks, rows, ends = oracle_batch
    for k, cuts in enumerate(([0, N_SENT], [0, 1234, N_SENT])):  # one shard; two shards (the gathered slots of two ranks)
        d = str(tmp_path / f"all{k}")
        bench.dump_outputs(d, scattered_parts(toks, ends, cuts, seed=k))
        got = load(d)
        assert np.array_equal(got["tok_cnt"], np.diff(ends))
        assert np.array_equal(got["sentences"], np.arange(N_SENT))
        assert np.array_equal(got["tokens"], rows)


def test_dump_outputs_samples_a_larger_output_the_same_way_every_time(bench, oracle_batch, tmp_path, monkeypatch):
    toks, rows, ends = oracle_batch
    budget = 16 * N_SENT + rows.nbytes // 3
    monkeypatch.setattr(bench, "DUMP_BYTES", budget)
    got = []
    for k, cuts in enumerate(([0, N_SENT], [0, 1234, N_SENT])):  # (another arrival order, another sharding: the same files)
        d = str(tmp_path / f"sample{k}")
        bench.dump_outputs(d, scattered_parts(toks, ends, cuts, seed=10 + k))
        got.append(load(d))
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= budget + 3 * 128  # (.npy headers)
    a, b = got
    assert all(np.array_equal(a[f], b[f]) for f in a)
    pick = a["sentences"].astype(np.int64)
    assert 0 < len(pick) < N_SENT and np.all(np.diff(pick) > 0)
    assert len(a["tokens"]) * 3 > len(rows) // 2  # the budget is used, not a token sample of a few sentences
    assert np.array_equal(a["tok_cnt"], np.diff(ends))
    assert np.array_equal(a["tokens"], np.concatenate([rows[ends[s]:ends[s + 1]] for s in pick]))


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_what_the_oracle_computes(oracle_batch, tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` without --full: the result line with ms_per_step and none of the --full legs, and
    --dump-outputs = the oracle's records of the same seeded corpus."""
    _, rows, ends = oracle_batch
    d = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dict", "small",
           "--sentences", str(N_SENT), "--dump-outputs", d]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    r = json.loads(lines[0])
    assert r["metric"] == "sentences/sec" and r["unit"] == "sentences/s" and r["higher_is_better"] is True and r["dtype"]
    assert r["steps"] == 2 and r["warmup"] == 1 and r["ms_per_step"] > 0
    assert abs(r["value"] - N_SENT / (r["ms_per_step"] * 1e-3)) <= 1e-3 * r["value"]  # (both are rounded in the line)
    assert r["tokens_per_step"] == len(rows)
    assert r["full"] is False
    for leg in ("parity_vs_oracle_sample", "roofline", "cpu_baseline", "cpu_baseline_all_cores", "suite", "worker_loop",
                "two_batches_in_flight", "host_to_host", "format"):
        assert r[leg] is None, leg
    got = load(d)
    assert np.array_equal(got["tok_cnt"], np.diff(ends))
    assert np.array_equal(got["sentences"], np.arange(N_SENT))
    assert np.array_equal(got["tokens"], rows)


@pytest.mark.gpu
def test_two_ranks_dump_what_one_rank_dumps(oracle_batch, tmp_path):
    """--gpus 2 (both ranks on the one GPU, gloo: the hooks of tests/test_distributed_gpu.py): rank 0 writes the gathered slots of the
    last step, every rank's shard in corpus order -- the same files as the single-GPU run of the same corpus."""
    _, rows, ends = oracle_batch
    d = str(tmp_path / "dump2")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(VBT_BENCH_BACKEND="gloo", VBT_BENCH_SINGLE_DEVICE="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--dict", "small",
           "--sentences", str(N_SENT), "--dump-outputs", d]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert r["n_gpus"] == 2 and r["gather"]["delivered_all_shards"] is True and r["tokens_per_step"] == len(rows)
    got = load(d)
    assert np.array_equal(got["tok_cnt"], np.diff(ends))
    assert np.array_equal(got["sentences"], np.arange(N_SENT))
    assert np.array_equal(got["tokens"], rows)
