#!/usr/bin/env python3
"""Developer aid: vbt_batch_format call by call on one headline-sized batch (cold / warm buffer, thread counts).
usage (GPU box): python tools/format_bench.py [threads ...]
                 python tools/format_bench.py --wakati    (wakati text: host formatter route against the device route)
                 python tools/format_bench.py --mecab     (MeCab-format text: the same two routes)
                 python tools/format_bench.py --detail    (detail text: the same two routes)"""
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one():
    import vibrato_amd as V
    from vibrato_amd import _native as N
    from tools import synth
    sd = synth.SynthDict("unidic")
    dv = V.SystemDictionaryBuilder.from_readers_binmatrix(sd.lex, sd.matrix, sd.num_right, sd.num_left, sd.char_def, sd.unk)
    tok = V.Tokenizer(dv)
    text, offs = sd.sentences(100000, "lognormal_40")
    b = tok.tokenize_batch(text=text, offsets=offs)
    L = N.lib()
    ts = []
    for i in range(8):
        p, n = C.c_void_p(), C.c_size_t()
        t = time.perf_counter()
        N.check(L.vbt_batch_format(b._h, 0, C.byref(p), C.byref(n)))
        ts.append((time.perf_counter() - t) * 1e3)
        L.vbt_free(p)
    print(f"threads={os.environ.get('VBT_FORMAT_THREADS', 'default')}: {n.value / 1e6:.1f} MB; ms per call: " + " ".join(f"{x:.2f}" for x in ts)
          + f"; best {n.value / min(ts) / 1e6:.1f} GB/s")


def routes(mode, rounds=12, calls=8):
    """Text in -> wakati / MeCab-format / detail text out on one headline-sized batch, one caller thread, one process: the host route
    (vbt_tokenize_batch + vbt_batch_format + the frees) against the device route (vbt_tokenize_wakati / vbt_tokenize_mecab / vbt_tokenize_detail + vbt_free),
    alternating, `calls` calls per timed window; medians, the run-to-run spread of either route, the bytes that leave the device per
    batch, and ms_pack of the device-resident call (the fallback launch + the record packing, or + the three kernels of the text
    mode) with and without the text mode."""
    import statistics
    import numpy as np
    import torch
    import vibrato_amd as V
    from vibrato_amd import _native as N
    from tools import synth
    sd = synth.SynthDict("unidic")
    dv = V.SystemDictionaryBuilder.from_readers_binmatrix(sd.lex, sd.matrix, sd.num_right, sd.num_left, sd.char_def, sd.unk)
    tok = V.Tokenizer(dv)
    text, offs = sd.sentences(100000, "lognormal_40")
    n, L, h = len(offs) - 1, N.lib(), tok._handle()

    def host():
        b, p, ln = C.c_void_p(), C.c_void_p(), C.c_size_t()
        N.check(L.vbt_tokenize_batch(h, text.ctypes.data, offs.ctypes.data, n, C.byref(b)))
        N.check(L.vbt_batch_format(b, {"mecab": 0, "wakati": 1, "detail": 2}[mode], C.byref(p), C.byref(ln)))
        nt = L.vbt_batch_total_tokens(b)
        L.vbt_free(p)
        L.vbt_batch_free(b)
        return ln.value, n * 8 + nt * 24

    def device():
        p, ln = C.c_void_p(), C.c_size_t()
        N.check(getattr(L, "vbt_tokenize_" + mode)(h, text.ctypes.data, offs.ctypes.data, n, C.byref(p), C.byref(ln), None))
        L.vbt_free(p)
        return ln.value, ln.value

    ref = tok.tokenize_batch(text=text, offsets=offs).format(mode).encode()
    assert getattr(tok, "tokenize_" + mode)(text=text, offsets=offs) == ref  # (the same bytes at the size that is timed)
    for _ in range(3):  # warm-up: pools, pinned blocks, the renumbered image
        host(), device()
    tok.wait_connid_reorder()
    ms = {"host": [], "device": []}
    for _ in range(rounds):
        for name, f in (("host", host), ("device", device)):
            t = time.perf_counter()
            for _ in range(calls):
                out_bytes, copied = f()
            ms[name].append((time.perf_counter() - t) * 1e3 / calls)
            ms[name + "_bytes"] = (out_bytes, copied)
    for name in ("host", "device"):
        v = ms[name]
        med = statistics.median(v)
        print(f"{name:6s}: median {med:.3f} ms per batch = {n / med / 1e3:.1f} M sentences/s; min {min(v):.3f} max {max(v):.3f} (spread {100 * (max(v) - min(v)) / med:.1f} %); "
              f"output {ms[name + '_bytes'][0] / 1e6:.1f} MB, copied out {ms[name + '_bytes'][1] / 1e6:.1f} MB")
    d_text, d_offs = torch.from_numpy(text).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda()
    ws = tok.workspace(n, len(text))
    ws.set_timing(True)
    for on in (False, True):
        if mode == "wakati":
            ws.set_wakati(on)
        elif mode == "mecab":
            ws.set_mecab(on, cap_bytes=len(ref))
        else:
            ws.set_detail(on, cap_bytes=len(ref))
        v = []
        for _ in range(10):
            ws.run(d_text.data_ptr(), d_offs.data_ptr(), n, len(text), torch.cuda.current_stream().cuda_stream)
            v.append(ws.stats()["ms_pack"])
        print(f"ms_pack, device-resident call, {mode} mode {'on (records not packed)' if on else 'off'}: median {statistics.median(v[2:]):.4f} ms")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] in ("--wakati", "--mecab", "--detail"):
        routes(sys.argv[1][2:])
    elif len(sys.argv) > 1 and sys.argv[1] == "--one":
        one()
    else:
        for t in (sys.argv[1:] or ["16", "32", "64", "128"]):
            subprocess.run([sys.executable, os.path.abspath(__file__), "--one"], env=dict(os.environ, VBT_FORMAT_THREADS=t))
