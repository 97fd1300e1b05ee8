"""One-call host-to-host rate of Tokenizer.tokenize_sample on BASELINE config 3's workload (unidic-shaped dictionary, 100 000
sentences, lognormal lengths) at T = 1000 for n_samples in {1, 4, 16} (argv[1] = sentences, argv[2] = synthetic dictionary), with the
same run's tokenize_nbest N = 1 and tokenize_marginal at min_prob 0 and 0.01 -- which share the generator phases, the marginals the
forward sweep too -- beside it: best / median of 3 after a warm-up.  Prints one JSON line; the numbers of DESIGN.md 3.4h /
profiles/EXPERIMENTS.md come from here.  Needs an MI355X."""
import json
import sys
import time

import vibrato_amd as V
from tools import synth


def best_of(f, reps):
    f()  # warm-up: workspaces, pinned blocks, the renumbered device image
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t)
    return min(ts), sorted(ts)[len(ts) // 2], r


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    sd = synth.SynthDict(sys.argv[2] if len(sys.argv) > 2 else "unidic")
    dv = V.SystemDictionaryBuilder.from_readers_binmatrix(sd.lex, sd.matrix, sd.num_right, sd.num_left, sd.char_def, sd.unk)
    text, offs = sd.sentences(n, "lognormal_40", seed=synth.SEED)
    tok = V.Tokenizer(dv, device=0)
    tok.calibrate(text=text, offsets=offs)
    out = {"sentences": n, "bytes": int(len(text))}

    def rate(lo, med):
        return {"best_sentences_per_s": round(n / lo), "median_sentences_per_s": round(n / med)}

    lo, med, _ = best_of(lambda: tok.tokenize_nbest(text=text, offsets=offs, n=1), 3)
    out["nbest_1"] = rate(lo, med)
    for p in (0.0, 0.01):
        lo, med, r = best_of(lambda: tok.tokenize_marginal(text=text, offsets=offs, temperature=1000.0, min_prob=p), 3)
        out[f"marginal_min_prob_{p:g}"] = dict(rate(lo, med), nodes=int(r.arrays()[0][-1]))
    for k in (1, 4, 16):
        lo, med, r = best_of(lambda: tok.tokenize_sample(text=text, offsets=offs, temperature=1000.0, n_samples=k, seed=1), 3)
        out[f"sample_{k}"] = dict(rate(lo, med), slab_share=round(r.slab_sentences() / n, 4), tokens=int(r.arrays()[1][-1]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
