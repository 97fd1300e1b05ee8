"""Builds vibrato_amd/lib/libvibrato_hip.so in-tree with hipcc for gfx950 (MI355X only): one object per translation unit,
compiled in parallel, then linked."""
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
SO = os.path.join(LIBDIR, "libvibrato_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# host code, then the kernels: gen.hip (validate_batch, generators, work lists), lattice.hip (the sweep, the resident Worker
# kernel), fused.hip (the single-kernel fallback), pack.hip (token compaction, connector expansion), wakati.hip (segmented text rendered on the device), mecab.hip (MeCab-format text rendered on the device), detail.hip (detail text rendered on the device), format.cpp + format.hip (user-defined output formats: their compiler, and the field index and the lines rendered on the device), split.hip (raw bytes cut into lines on the device), nbest.hip (the K best paths per sentence), marginal.hip (the posterior probability of every lattice node), sample.hip (whole paths sampled from that distribution), engine.hip (Tokenizer, Workspace)
SOURCES = ["dict.cpp", "connector.cpp", "dictio.cpp", "format.cpp", "capi.cpp", "engine.hip", "gen.hip", "lattice.hip", "fused.hip", "pack.hip", "wakati.hip", "mecab.hip", "detail.hip", "format.hip", "split.hip", "nbest.hip", "marginal.hip", "sample.hip"]
# every header under csrc/ (sweep_asm.hpp -- the hottest code -- was once missing from a hand-written list) + the C ABI
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".hpp")) + ["../../include/vibrato_hip.h"]
# per source file, on top of FLAGS (wakati.hip, mecab.hip, detail.hip, format.hip, split.hip, nbest.hip, marginal.hip, sample.hip: the packed fp32 instructions stay out of new device code)
NO_PACKED_FP32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
EXTRA_FLAGS = {"wakati.hip": NO_PACKED_FP32, "mecab.hip": NO_PACKED_FP32, "detail.hip": NO_PACKED_FP32, "format.hip": NO_PACKED_FP32, "split.hip": NO_PACKED_FP32, "nbest.hip": NO_PACKED_FP32, "marginal.hip": NO_PACKED_FP32, "sample.hip": NO_PACKED_FP32}
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall", "-Wno-unused-result", "-Wno-unused-function"]


def needs_build():
    if not os.path.exists(SO):
        return True
    t = os.path.getmtime(SO)
    return any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in SOURCES + HEADERS)


def variant_so(variant):
    return os.path.join(LIBDIR, f"libvibrato_hip{('_' + variant) if variant else ''}.so")


def build(force=False, verbose=False, variant="", defines=()):
    """variant/defines: developer A/B builds (lib/libvibrato_hip_<variant>.so with -D flags),
    selected at load time with VBT_LIB_VARIANT=<variant>."""
    so = variant_so(variant)
    if not variant and not force and not needs_build():
        return so
    os.makedirs(LIBDIR, exist_ok=True)
    with tempfile.TemporaryDirectory(prefix="vbt_build_") as tmp:
        def compile_one(f):
            obj = os.path.join(tmp, f + ".o")
            cmd = [HIPCC] + FLAGS + EXTRA_FLAGS.get(f, []) + ["-D" + d for d in defines] + ["-x", "hip", "-c", os.path.join(CSRC, f), "-o", obj]
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            subprocess.check_call(cmd)
            return obj
        with ThreadPoolExecutor(max_workers=min(len(SOURCES), os.cpu_count() or 1)) as ex:
            objs = list(ex.map(compile_one, SOURCES))
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-ldl", "-lhsa-runtime64", "-o", so]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
    return so


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose="--verbose" in sys.argv)
    print(SO)
