"""Per-kernel resources of one HIP source file, from the compiler alone (no GPU): VGPRs, SGPRs, LDS, scratch, occupancy
(-Rpass-analysis=kernel-resource-usage) and the instruction count of each kernel's gfx950 disassembly (--save-temps).

    python tools/isa_resources.py <tree> [file.hip]     # <tree>: a checkout's root (default file: lbvh_path.hip)

One line per kernel, demangled name first, so that two trees' listings can be compared line by line (profiles/ray_queries/)."""
import os
import re
import subprocess
import sys
import tempfile

FIELDS = (("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occ"),
          ("LDS Size [bytes/block]", "lds"))


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def resources(tree, src="lbvh_path.hip"):
    csrc = os.path.join(os.path.abspath(tree), "unitysimpleraytracing_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
               "-Wall", "-Wno-unused-function", "-Rpass-analysis=kernel-resource-usage", "--save-temps", "-c",
               os.path.join(csrc, src), "-o", os.path.join(tmp, "out.o")]
        remarks = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True, check=True).stderr
        asm = open(os.path.join(tmp, src.replace(".hip", "") + "-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    kernels, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        for key, short in FIELDS:
            m = re.search(re.escape(key) + r": (\S+)", line)
            if m and cur is not None:
                cur[short] = m.group(1)
    for name, row in kernels.items():
        body = asm[asm.index(f"\n{name}:"):]
        body = body[: body.index(".Lfunc_end")]
        row["insts"] = sum(1 for ln in body.splitlines()[1:] if re.match(r"\s+[a-z_][a-z0-9_]*", ln) and not ln.strip().startswith("."))
    pretty = demangle(list(kernels))
    return {pretty[n]: r for n, r in kernels.items()}


def main():
    tree = sys.argv[1] if len(sys.argv) > 1 else "."
    src = sys.argv[2] if len(sys.argv) > 2 else "lbvh_path.hip"
    for name, r in sorted(resources(tree, src).items()):
        print(f"{name}: " + " ".join(f"{k}={r.get(k, '?')}" for k in ("vgpr", "sgpr", "lds", "scratch", "occ", "insts")))


if __name__ == "__main__":
    main()
