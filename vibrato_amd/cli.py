"""`tokenize`-compatible command line (reference: tokenize/src/main.rs:31-132).

    python -m vibrato_amd.cli -i system.dic.zst [-u user.csv] [-O mecab|wakati|detail] [-F FMT [-U FMT] [-B FMT] [-E FMT]] [-S] [-M N] < lines.txt

-i takes what the reference's CLI takes -- a dictionary written by Dictionary::write, zstd-compressed or not
(tokenize/src/main.rs:34,59-60) -- or a directory of MeCab-format sources (lex.csv, matrix.def, char.def, unk.def).
--compile-to PATH writes the loaded dictionary back out as system.dic.zst (compile/src/main.rs:98).  Lines are read with the semantics of BufRead::lines()
(`\\n` / `\\r\\n` stripped) and tokenized in blocks of --block lines per GPU batch; the bytes
written are exactly those of the reference CLI for the same mode.
`-O marginal --temperature T [--min-prob P]` (no counterpart in the reference; MeCab's -m with -t) prints every lattice node
whose posterior probability is at least P as `surface\\tfeature\\tprob`, then `EOS`.
`-O sample --temperature T [--samples N] [--seed S]` prints N segmentations per sentence drawn from P(path) ~ exp(-cost / T), one
line of space-separated surfaces each, then `EOS` (block k of the input is drawn with seed S + the lines in front of it).
-F/--node-format (with -U/--unk-format, -B/--bos-format, -E/--eos-format; MeCab's options of those names, the directives are listed
in include/vibrato_hip.h) replaces the output mode by a format of the caller's, rendered on the device.
"""
import argparse
import os
import sys

from . import api


def read_sources(d):
    out = []
    for f in ("lex.csv", "matrix.def", "char.def", "unk.def"):
        with open(os.path.join(d, f), "rb") as fh:
            out.append(fh.read())
    return out


def render_marginal(d, lines, mg):
    """-O marginal: "surface\\tfeature\\tprob" per reported lattice node (lattice order), "EOS" per sentence -- formatted here from
    the arrays of Tokenizer.tokenize_marginal."""
    node_off, _, nodes = mg.arrays()
    feature, out = {}, []
    for s, line in enumerate(lines):
        for g in nodes[int(node_off[s]):int(node_off[s + 1])]:
            w = int(g["word_idx"])
            if w not in feature:
                feature[w] = d.word_feature(w >> 30, w & 0x3FFFFFFF).encode("utf-8")
            out += [line[int(g["start_byte"]):int(g["end_byte"])], b"\t", feature[w], b"\t%.6f\n" % float(g["prob"])]
        out.append(b"EOS\n")
    return b"".join(out)


def render_sample(lines, sm):
    """-O sample: per sentence one line of space-separated surfaces per sampled path, then "EOS" -- formatted here from the arrays
    of Tokenizer.tokenize_sample."""
    path_off, tok_off, _, _, toks = sm.arrays()
    out = []
    for s, line in enumerate(lines):
        for p in range(int(path_off[s]), int(path_off[s + 1])):
            recs = toks[int(tok_off[p]):int(tok_off[p + 1])]
            out += [b" ".join(line[int(g["start_byte"]):int(g["end_byte"])] for g in recs), b"\n"]
        out.append(b"EOS\n")
    return b"".join(out)


def main(argv=None, stdin=None, stdout=None):
    ap = argparse.ArgumentParser(prog="tokenize", description="Predicts morphemes")
    ap.add_argument("-i", "--sysdic", required=True, help="System dictionary (in zstd), or a directory with lex.csv, matrix.def, char.def, unk.def")
    ap.add_argument("--compile-to", default=None, help="also write the dictionary as system.dic.zst (zstd level 19) to this path")
    ap.add_argument("-u", "--userlex-csv", default=None, help="User lexicon file.")
    ap.add_argument("-O", "--output-mode", default="mecab", choices=["mecab", "wakati", "detail", "marginal", "sample"])
    ap.add_argument("-F", "--node-format", default=None, help="per token, e.g. '%%m\\t%%f[0]\\n' (MeCab's directives; rendered on the device, instead of -O)")
    ap.add_argument("-U", "--unk-format", default=None, help="per unknown word (default: the node format)")
    ap.add_argument("-B", "--bos-format", default="", help="in front of every sentence (literals and escapes)")
    ap.add_argument("-E", "--eos-format", default="EOS\\n", help="behind every sentence (literals and escapes)")
    ap.add_argument("--temperature", type=float, default=None, help="marginal and sample mode: P(path) ~ exp(-cost / temperature), in cost units (required there)")
    ap.add_argument("--min-prob", type=float, default=0.0, help="marginal mode: report the lattice nodes whose probability is at least this")
    ap.add_argument("--samples", type=int, default=1, help="sample mode: paths drawn per sentence (1 .. 64)")
    ap.add_argument("--seed", type=int, default=0, help="sample mode: seed of the draw")
    ap.add_argument("-S", "--ignore-space", action="store_true", help="Ignores white spaces in input strings.")
    ap.add_argument("-M", "--max-grouping-len", type=int, default=None, help="Maximum length of unknown words.")
    ap.add_argument("--block", type=int, default=65536, help="lines per GPU batch")
    ap.add_argument("--device", type=int, default=-1)
    args = ap.parse_args(argv)
    stdin = stdin or sys.stdin.buffer
    stdout = stdout or sys.stdout.buffer

    print("Loading the dictionary...", file=sys.stderr)
    if os.path.isdir(args.sysdic):
        d = api.SystemDictionaryBuilder.from_readers(*read_sources(args.sysdic))
    else:
        d = api.Dictionary.read(args.sysdic)
    if args.compile_to:
        with open(args.compile_to, "wb") as fh:
            d.write(fh, zstd_level=19)
    if args.userlex_csv:
        with open(args.userlex_csv, "rb") as fh:
            d.reset_user_lexicon_from_reader(fh.read())
    tok = api.Tokenizer(d, device=args.device).ignore_space(args.ignore_space).max_grouping_len(args.max_grouping_len or 0)
    print("Ready to tokenize", file=sys.stderr)

    # Three stages, each on its own thread (the library calls release the GIL): this thread reads lines and cuts blocks, one thread
    # pushes block k + 1 through the GPU (vbt_tokenize_batch), one renders block k (vbt_batch_format) and writes it -- the formatter
    # of one block runs under the kernels and copies of the next.  Output order = input order (one block at a time per stage).
    # (on a single-device tokenizer the block's text is rendered on the device in every output mode -- Tokenizer.tokenize_wakati /
    # tokenize_mecab / tokenize_detail -- and the output stage only writes it; DESIGN.md 3.4a-c hold the measurements behind that)
    import queue
    import threading
    text_on_device = tok.num_devices() == 1 or args.output_mode in ("marginal", "sample")
    if args.node_format is not None:  # (the device route beat records + a host formatter)
        if tok.num_devices() != 1:
            ap.error("-F needs a single-device tokenizer")
        fmt = tok.compile_format(args.node_format, args.unk_format, args.bos_format, args.eos_format)
        text_on_device = True
        tokenize_text = lambda lines: tok.tokenize_format(lines, fmt)  # noqa: E731
    elif args.output_mode == "marginal":
        if args.temperature is None:
            ap.error("-O marginal needs --temperature")
        tokenize_text = lambda lines: render_marginal(d, lines, tok.tokenize_marginal(lines, args.temperature, args.min_prob))  # noqa: E731
    elif args.output_mode == "sample":
        if args.temperature is None:
            ap.error("-O sample needs --temperature")
        seen = [0]  # lines in front of the block (one block at a time passes the tokenize stage)

        def tokenize_text(lines):
            sm = tok.tokenize_sample(lines, args.temperature, args.samples, args.seed + seen[0])
            seen[0] += len(lines)
            return render_sample(lines, sm)
    else:
        tokenize_text = {"wakati": tok.tokenize_wakati, "mecab": tok.tokenize_mecab, "detail": tok.tokenize_detail}[args.output_mode]
    blocks, batches = queue.Queue(maxsize=2), queue.Queue(maxsize=2)
    failure = []

    def tokenize_stage():
        try:
            while True:
                lines = blocks.get()
                if lines is None:
                    break
                if not failure:
                    batches.put(tokenize_text(lines) if text_on_device else tok.tokenize_batch(lines))
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            failure.append(e)
            while blocks.get() is not None:  # (keep draining: the reader must not block on a full queue)
                pass
        batches.put(None)

    def output_stage():
        try:
            while True:
                b = batches.get()
                if b is None:
                    break
                if not failure:
                    if text_on_device:
                        stdout.write(b)
                    else:
                        b.format_into(stdout.write, args.output_mode)
        except BaseException as e:  # noqa: BLE001
            failure.append(e)
            while batches.get() is not None:
                pass

    # (daemon threads, and the sentinel is posted whatever happens to the reader -- an I/O error on stdin, a KeyboardInterrupt: the stages
    # then finish what is queued and the reader's exception is raised behind the join instead of an interpreter that hangs at exit)
    stages = [threading.Thread(target=tokenize_stage, daemon=True), threading.Thread(target=output_stage, daemon=True)]
    for t in stages:
        t.start()
    reader_error = None
    try:
        block = []
        for raw in stdin:
            if raw.endswith(b"\n"):
                raw = raw[:-1]
                if raw.endswith(b"\r"):
                    raw = raw[:-1]
            block.append(raw)
            if len(block) >= args.block:
                blocks.put(block)
                block = []
        if block:
            blocks.put(block)
    except BaseException as e:  # noqa: BLE001 -- re-raised below, behind the join
        reader_error = e
        failure.append(e)  # (the stages skip what is still queued)
    finally:
        blocks.put(None)
        for t in stages:
            t.join()
    if reader_error is not None:
        raise reader_error
    if failure:
        raise failure[0]
    stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
