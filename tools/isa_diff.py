#!/usr/bin/env python3
"""Per-kernel gfx950 instruction streams of one checkout's kernels against another's: shows that a change which adds instantiations
left the existing ones as they were (the logs profiles/*_isa_diff_vs_parent.txt).

    python tools/isa_diff.py OLD_TREE NEW_TREE [source.hip ...]      (default sources: kernels.hip layer_fused.hip)

Each source of each tree is compiled with `hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only`; a kernel's body is
its instructions from its label to the end of the function (.Lfunc_end), comments, directives and labels dropped and local label names replaced by one token
(they are numbered per file).  Kernels only in NEW_TREE are listed with their instruction, scratch, conversion and MFMA counts."""
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def bodies(tree, src, tmp, tag):
    if not os.path.exists(os.path.join(tree, "moe-infinity_amd", "csrc", src)):
        return {}  # a source one of the trees does not have: all of its kernels are new (or missing)
    out_s = os.path.join(tmp, f"{tag}_{src}.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out_s,
                    os.path.join(tree, "moe-infinity_amd", "csrc", src)], check=True, capture_output=True)
    lines = open(out_s).read().split("\n")
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\S+):", l)
        if not m:
            continue
        end = next((j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end")), None)  # (a kernel may hold several s_endpgm)
        if end is None:
            continue
        body = [x.strip() for x in lines[i + 1:end]]
        body = [x for x in body if x and not x.startswith((";", ".")) and not re.match(r"^\S+:$", x)]
        out[m.group(1)] = [re.sub(r"\.L[A-Za-z_]*\d+_\d+|\.Ltmp\d+|\.L__\S+", "L", x) for x in body]
    return out


def main(old, new, sources):
    with tempfile.TemporaryDirectory() as tmp:
        for src in sources:
            o, n = bodies(old, src, tmp, "old"), bodies(new, src, tmp, "new")
            same = [k for k in o if k in n and o[k] == n[k]]
            diff = [k for k in o if k in n and o[k] != n[k]]
            gone = [k for k in o if k not in n]
            added = [k for k in n if k not in o]
            print(f"{src}: parent kernels {len(o)}, identical instruction streams {len(same)}, different {len(diff)}, missing {len(gone)}, "
                  f"new {len(added)}")
            for k in diff:
                print("  DIFFERENT", k, len(o[k]), len(n[k]))
            for k in gone:
                print("  MISSING", k)
            for k in added:
                b = n[k]
                print("  new", k, "instr", len(b), "scratch", sum("scratch_" in x for x in b), "cvt_fp4",
                      sum(x.startswith("v_cvt_scalef32_pk_bf16_fp4") for x in b), "mfma", sum(x.startswith("v_mfma") for x in b))


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2]), sys.argv[3:] or ["kernels.hip", "layer_fused.hip"])
