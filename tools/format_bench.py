#!/usr/bin/env python3
"""Developer aid: vbt_batch_format call by call on one headline-sized batch (cold / warm buffer, thread counts).
usage (GPU box): python tools/format_bench.py [threads ...]
                 python tools/format_bench.py --wakati    (wakati text: host formatter route against the device route)
                 python tools/format_bench.py --mecab     (MeCab-format text: the same two routes)
                 python tools/format_bench.py --detail    (detail text: the same two routes)
                 python tools/format_bench.py --format    (compiled formats, format.hip: against mecab.hip, and against records + a numpy formatter)"""
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


def format_routes(rounds=12, calls=8):
    """Compiled formats (Tokenizer.tokenize_format) on one headline-sized batch, the protocol of routes(): (a) "%m\\t%H\\n" through the
    general renderer against (b) tokenize_mecab, the specialised kernel; (c) the field-cutting format "%m\\t%f[0],%f[1]\\n" through
    the general renderer against tokenize_batch + a host formatter -- numpy gathers over the records, the per-word "\\tf0,f1\\n"
    strings cut once outside the timed part.  Then ms_pack of the device-resident call in format mode, and the wall time of the
    first set_format of a new format object (the field index: allocation, format_index, the exception list read back)."""
    import csv
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
    f_mecab, f_cut = tok.compile_format("%m\t%H\n"), tok.compile_format("%m\t%f[0],%f[1]\n")
    d = tok.dictionary()
    words = [d.num_words(lx) for lx in range(3)]
    lex_base = np.cumsum([0] + words[:2]).astype(np.int64)
    tails = []
    for lx in range(3):
        for w in range(words[lx]):
            f = (next(csv.reader([d.word_feature(lx, w)]), None) or [""]) + ["", ""]
            tails.append(("\t" + f[0] + "," + f[1] + "\n").encode())
    tail_off = np.cumsum([0] + [len(t) for t in tails]).astype(np.int64)
    src = np.concatenate([text, np.frombuffer(b"".join(tails) + b"EOS\n", dtype=np.uint8)])  # every piece's source in one array
    offs64 = offs.astype(np.int64)

    def host_cut():
        b = tok.tokenize_batch(text=text, offsets=offs)
        recs, ends = b.tokens_in_order()
        ends = ends.astype(np.int64)
        cnt, nt = np.diff(ends), int(ends[-1])
        sid = np.repeat(np.arange(n, dtype=np.int64), cnt)
        row = lex_base[recs["word_idx"] >> 30] + (recs["word_idx"] & 0x3FFFFFFF)
        p_src, p_len = np.empty(2 * nt + n, dtype=np.int64), np.empty(2 * nt + n, dtype=np.int64)  # pieces in output order
        at = 2 * np.arange(nt, dtype=np.int64) + sid
        p_src[at], p_len[at] = offs64[sid] + recs["start_byte"], recs["end_byte"].astype(np.int64) - recs["start_byte"]
        p_src[at + 1], p_len[at + 1] = len(text) + tail_off[row], tail_off[row + 1] - tail_off[row]
        eos = 2 * ends[1:] + np.arange(n, dtype=np.int64)
        p_src[eos], p_len[eos] = len(text) + tail_off[-1], 4
        start = np.cumsum(p_len) - p_len
        out = src[np.repeat(p_src - start, p_len) + np.arange(int(start[-1] + p_len[-1]), dtype=np.int64)]
        return out, len(out), n * 8 + nt * 24

    def device(fmt):
        def call():
            p, ln = C.c_void_p(), C.c_size_t()
            if fmt is None:
                N.check(L.vbt_tokenize_mecab(h, text.ctypes.data, offs.ctypes.data, n, C.byref(p), C.byref(ln), None))
            else:
                N.check(L.vbt_tokenize_format(h, fmt._h, text.ctypes.data, offs.ctypes.data, n, C.byref(p), C.byref(ln), None))
            L.vbt_free(p)
            return None, ln.value, ln.value
        return call

    ref = tok.tokenize_mecab(text=text, offsets=offs)
    assert tok.tokenize_format(fmt=f_mecab, text=text, offsets=offs) == ref  # (the same bytes at the size that is timed)
    assert tok.tokenize_format(fmt=f_cut, text=text, offsets=offs) == host_cut()[0].tobytes()
    legs = (("(a) format %m\\t%H\\n, device", device(f_mecab)), ("(b) mecab.hip, device", device(None)), ("(c) %m\\t%f[0],%f[1]\\n, host", host_cut),
            ("(c) %m\\t%f[0],%f[1]\\n, device", device(f_cut)))
    for _ in range(3):  # warm-up: pools, pinned blocks, the renumbered image
        for _, f in legs:
            f()
    tok.wait_connid_reorder()
    ms, sizes = {name: [] for name, _ in legs}, {}
    for _ in range(rounds):
        for name, f in legs:
            t = time.perf_counter()
            for _ in range(calls):
                _, out_bytes, copied = f()
            ms[name].append((time.perf_counter() - t) * 1e3 / calls)
            sizes[name] = (out_bytes, copied)
    for name, _ in legs:
        v = ms[name]
        med = statistics.median(v)
        print(f"{name:34s}: median {med:.3f} ms per batch; min {min(v):.3f} max {max(v):.3f} (spread {100 * (max(v) - min(v)) / med:.1f} %); "
              f"output {sizes[name][0] / 1e6:.1f} MB, copied out {sizes[name][1] / 1e6:.1f} MB")
    d_text, d_offs = torch.from_numpy(text).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda()
    ws = tok.workspace(n, len(text))
    ws.set_timing(True)
    for name, fmt in (("off", None), ("%m\\t%H\\n", f_mecab), ("%m\\t%f[0],%f[1]\\n", f_cut)):
        ws.set_format(fmt, cap_bytes=len(ref) if fmt else 0)
        v = []
        for _ in range(10):
            ws.run(d_text.data_ptr(), d_offs.data_ptr(), n, len(text), torch.cuda.current_stream().cuda_stream)
            v.append(ws.stats()["ms_pack"])
        print(f"ms_pack, device-resident call, format mode {name}: median {statistics.median(v[2:]):.4f} ms")
    ws.set_format(None)
    for node in ("%f[0]\n", "%f[0],%f[1],%f[2],%f[3],%f[4],%f[5],%f[6],%f[7]\n"):
        fresh = tok.compile_format(node)
        t = time.perf_counter()
        ws.set_format(fresh, cap_bytes=len(ref))
        print(f"first set_format of a new format with {node.count('%f')} field(s) over {sum(words)} words: {(time.perf_counter() - t) * 1e3:.2f} ms")
        ws.set_format(None)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--format":
        format_routes()
    elif len(sys.argv) > 1 and sys.argv[1] in ("--wakati", "--mecab", "--detail"):
        routes(sys.argv[1][2:])
    elif len(sys.argv) > 1 and sys.argv[1] == "--one":
        one()
    else:
        for t in (sys.argv[1:] or ["16", "32", "64", "128"]):
            subprocess.run([sys.executable, os.path.abspath(__file__), "--one"], env=dict(os.environ, VBT_FORMAT_THREADS=t))
