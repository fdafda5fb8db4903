"""In-tree build of the gfx950 kernel library (libcocos_hip.so) and of the C oracle.

`hipcc --offload-arch=gfx950` cross-compiles without a GPU, so this runs in the CPU-only build
container; the resulting .so files are git-ignored but travel to the GPU box with the snapshot.
No cmake/ninja: a handful of translation units, compiled in parallel, linked once.
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
CSRC_DIR = os.path.join(PKG_DIR, "csrc")
LIB_DIR = os.path.join(PKG_DIR, "lib")
#: COCOS_LIB_NAME builds a second library next to the product one (e.g. a -DCOCOS_DEBUG_TIMING build for
#: tools/phase_timing_f16x3.py); cocosnet_amd._lib loads it when COCOS_LIB_PATH points at it
LIB_PATH = os.path.join(LIB_DIR, os.environ.get("COCOS_LIB_NAME", "libcocos_hip.so"))
OBJ_DIR = os.path.join(LIB_DIR, "obj" + ("" if "COCOS_LIB_NAME" not in os.environ else "_" + os.environ["COCOS_LIB_NAME"]))

HIP_SOURCES = [
    "api_common.hip",
    "center_l2norm.hip",
    "corr_fused_fwd.hip",
    "corr_fused_fwd_f16x3.hip",
    "split_f16.hip",
    "plane_prep.hip",
    "corr_fused_bwd_f16x3.hip",
    "hgemm_f16x3.hip",
    "corr_fused_bwd.hip",
    "corr_fused_bwd_saved.hip",
    "sgemm_mfma.hip",
    "sgemm_f16x3.hip",
    "proj_stream_f16x3.hip",
    "proj_dw_f16x3.hip",
    "proj_norm_f16x3.hip",
    "proj_bwd_f16x3.hip",
    "box3_unfold.hip",
    "box3_fused_f16x3.hip",
    "unfold3_stats.hip",
    "logits_softmax_warp.hip",
    "logits_softmax_warp_f16x3.hip",
    "row_softmax.hip",
    "wta_scale.hip",
    "pono_spade.hip",
    "instnorm_prelu.hip",
    "instnorm_split.hip",
    "label_conv.hip",
    "upsample_nearest.hip",
    "warp_values.hip",
    "warp_head.hip",
    "contextual_rows.hip",
    "contextual_fused_f16x3.hip",
    "conv_f16x3.hip",
    "conv_nhwc_bf16.hip",
    "spade_modulate.hip",
    "norm_spade.hip",
    "vgg_glue.hip",
    "loss_reduce.hip",
    "optim_step.hip",
    "weight_prepare_multi.hip",
    "reflect_pad.hip",
    "spectral_norm.hip",
    "gather_warp.hip",
    "corr_topk_f16x3.hip",
    "row_topk_lse.hip",
    "plane_pair.hip",
    "patchmatch_f16x3.hip",
    "patchmatch_box3.hip",
    "corr_match_mutual_f16x3.hip",
    "corr_lse_bwd_f16x3.hip",
    "corr_topk_bias_f16x3.hip",
    "box3_pair.hip",
    "box3_lse_bwd_f16x3.hip",
]
HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc",
             "-Wall", "-Wno-unused-function"]
#: per-file additions.  proj_dw: 224 accumulator registers per lane — with the default AGPR form of the MFMA results
#: hipcc also parks the staged global loads in the accumulator file, runs out of it and spills accumulators to
#: scratch inside the k loop (every reload is an s_waitcnt vmcnt(0): the prefetch is gone); VGPR form has no spills.
FILE_FLAGS = {"proj_dw_f16x3.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"]}


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (looked at $HIPCC, PATH, /opt/rocm/bin)")


def _flags():
    return HIP_FLAGS + os.environ.get("COCOS_EXTRA_HIPFLAGS", "").split()


def _digest(paths) -> str:
    h = hashlib.sha256()
    for p in sorted(paths):
        with open(p, "rb") as f:
            # file NAME, not the absolute path: the stamp must stay valid when the tree is copied elsewhere
            # (the prebuilt .so travels to the GPU box and must not be rebuilt there on every import)
            h.update(os.path.basename(p).encode())
            h.update(f.read())
    h.update(" ".join(_flags()).encode())
    h.update(repr(sorted(FILE_FLAGS.items())).encode())
    return h.hexdigest()


def build_hip(force: bool = False, verbose: bool = True) -> str:
    """Compile every HIP translation unit for gfx950 and link libcocos_hip.so. Returns its path."""
    os.makedirs(OBJ_DIR, exist_ok=True)
    srcs = [os.path.join(CSRC_DIR, s) for s in HIP_SOURCES]
    # every header under csrc/, found by listing it: one left off a hand-kept list would not enter the stamp, and editing it would
    # leave a stale library in use
    deps = srcs + sorted(os.path.join(CSRC_DIR, h) for h in os.listdir(CSRC_DIR) if h.endswith(".h")) + [
        os.path.join(REPO_DIR, "include", "cocos_hip.h")]
    stamp = LIB_PATH + ".sha256"      # next to the library: it travels with it (obj/ does not have to)
    want = _digest(deps)
    if (not force and os.path.exists(LIB_PATH) and os.path.exists(stamp)
            and open(stamp).read().strip() == want):
        return LIB_PATH
    hipcc = _hipcc()
    headers = [d for d in deps if not d.endswith(".hip")]

    def compile_one(src: str) -> str:
        # per-object stamp (source + every header + flags): editing one kernel file recompiles one translation unit
        obj = os.path.join(OBJ_DIR, os.path.basename(src) + ".o")
        ostamp, owant = obj + ".sha256", _digest([src] + headers)
        if not force and os.path.exists(obj) and os.path.exists(ostamp) and open(ostamp).read().strip() == owant:
            return obj
        cmd = [hipcc, *_flags(), *FILE_FLAGS.get(os.path.basename(src), []), "-c", src, "-o", obj]
        if verbose:
            print("[build]", " ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        with open(ostamp, "w") as f:
            f.write(owant)
        return obj

    with ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        objs = list(ex.map(compile_one, srcs))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH, *objs]
    if verbose:
        print("[build]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    with open(stamp, "w") as f:
        f.write(want)
    return LIB_PATH


def compile_check(sources=("upsample_nearest.hip", "wta_scale.hip"), verbose: bool = True) -> None:
    """Compile a couple of small translation units from scratch with the product flags into a temporary directory and check
    that the objects carry gfx950 code — `build_hip()` is a no-op when the shipped library's stamp matches the sources
    (the driver's build() then did not exercise the compiler at all).  ~10 s; `python -m cocosnet_amd.build
    --force` rebuilds everything."""
    import tempfile
    try:
        hipcc = _hipcc()
    except RuntimeError:
        # a host that only carries the prebuilt library (its stamp matched, or build_hip() would have raised already): nothing to
        # exercise — say so instead of failing an import-only deployment
        if verbose:
            print("[build] compile check skipped: no hipcc on this host (prebuilt library with a matching stamp is in use)", flush=True)
        return
    with tempfile.TemporaryDirectory(prefix="cocos_cc_") as tmp:
        for name in sources:
            src, obj = os.path.join(CSRC_DIR, name), os.path.join(tmp, name + ".o")
            cmd = [hipcc, *_flags(), *FILE_FLAGS.get(name, []), "-c", src, "-o", obj]
            if verbose:
                print("[build] compile check:", " ".join(cmd), flush=True)
            subprocess.run(cmd, check=True)
            blob = open(obj, "rb").read()
            if b"gfx950" not in blob or len(blob) < 4096:
                raise RuntimeError(f"compile check: {obj} holds no gfx950 code object")


def build_oracle(verbose: bool = True) -> None:
    """Nothing to compile: the oracle under oracle/ is numpy / torch, and the reference it is pinned against is pure
    Python (no oracle/_ref build).  Kept because __graft_entry__.build() calls it as the "build the checker" step; it
    only checks that the directory has its Python files (the package never imports it)."""
    odir = os.path.join(REPO_DIR, "oracle")
    have = [f for f in os.listdir(odir) if f.endswith(".py")] if os.path.isdir(odir) else []
    if len(have) < 2:
        raise FileNotFoundError(f"{odir}: the CPU restatements are missing")
    if verbose:
        print(f"[build] oracle: {len(have)} Python files present (nothing to compile)", flush=True)


if __name__ == "__main__":
    print(build_hip(force="--force" in sys.argv))
    build_oracle()
