"""Per-kernel resources of one HIP source file, from the compiler alone (no GPU): VGPRs, SGPRs, LDS, scratch, occupancy
(-Rpass-analysis=kernel-resource-usage) and the instruction count of each kernel's gfx950 disassembly (--save-temps).

    python tools/isa_resources.py <tree> [file.hip]     # <tree>: a checkout's root (default file: lbvh_path.hip)

One line per kernel, demangled name first, so that two trees' listings can be compared line by line (profiles/ray_queries/).

    python tools/isa_resources.py --compare <tree a> <tree b> <file.hip>

The gate for a change that must leave the device code alone: both trees' file is compiled for the device only, with the
flags of each tree's csrc/Makefile, and every kernel's instruction stream is compared as text — comments and directive lines dropped,
local labels (.LBB...) folded to one token, so that moved or renumbered source does not show.  One line per kernel, `same` or
`DIFFERENT`, `missing` for a kernel only <tree a> has and `extra` for one only <tree b> has; the exit status is 1 unless every line
says `same`.

    python tools/isa_resources.py --compare <tree a> <tree b>

The same over every .hip of each tree's own SRCS (csrc/Makefile), the kernels of a tree pooled by mangled name: a kernel that moved
to another file is `same` where it is found (`old.hip -> new.hip`).  A kernel that two files of one tree hold is `duplicate` and
fails the run like a difference: every kernel is instantiated in one translation unit."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

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


def makefile_flags(csrc):
    m = re.search(r"^CXXFLAGS\s*\?=\s*(.+)$", open(os.path.join(csrc, "Makefile")).read(), re.M)
    return m.group(1).split()


def instruction_streams(tree, src):
    """{mangled kernel name: its instructions, normalised, one per line}"""
    csrc = os.path.join(os.path.abspath(tree), "unitysimpleraytracing_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "device.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950"] + makefile_flags(csrc) +
                       ["--offload-device-only", "-S", os.path.join(csrc, src), "-o", out], cwd=tmp, capture_output=True, text=True, check=True)
        asm = open(out).read()
    streams = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M):
        body = asm[asm.index(f"\n{name}:") + 1:]
        body = body[: body.index(".Lfunc_end")]
        lines = []
        for ln in body.splitlines()[1:]:
            ln = re.sub(r"\.LBB\w+", ".LBB", ln.split(";")[0]).strip()
            if ln and (ln == ".LBB:" or not ln.startswith(".")):
                lines.append(" ".join(ln.split()))
        streams[name] = "\n".join(lines)
    return streams


def makefile_srcs(csrc):
    m = re.search(r"^SRCS\s*:=\s*(.+)$", open(os.path.join(csrc, "Makefile")).read(), re.M)
    return m.group(1).split()


def pooled_streams(tree):
    """Every .hip of the tree's own SRCS: ({mangled kernel name: (file, instructions)}, [(name, file, other file)] for a kernel two files hold)"""
    srcs = makefile_srcs(os.path.join(os.path.abspath(tree), "unitysimpleraytracing_amd", "csrc"))
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        per_file = list(pool.map(lambda src: instruction_streams(tree, src), srcs))
    kernels, twice = {}, []
    for src, streams in zip(srcs, per_file):
        for name, text in streams.items():
            if name in kernels:
                twice.append((name, kernels[name][0], src))
            else:
                kernels[name] = (src, text)
    return kernels, twice


def compare(tree_a, tree_b, src=None):
    if src:
        a = {name: (src, text) for name, text in instruction_streams(tree_a, src).items()}
        b = {name: (src, text) for name, text in instruction_streams(tree_b, src).items()}
        twice = []
    else:
        (a, twice_a), (b, twice_b) = pooled_streams(tree_a), pooled_streams(tree_b)
        twice = [(tree_a,) + t for t in twice_a] + [(tree_b,) + t for t in twice_b]
    pretty = demangle(sorted(set(a) | set(b) | {t[1] for t in twice}))
    bad, per_file = len(twice), {}
    for tree, name, first, second in twice:
        print(f"{first} + {second}: duplicate {pretty[name]}  in {tree}")
    for name in sorted(set(a) | set(b), key=lambda n: ((a.get(n) or b[n])[0], pretty[n])):
        verdict = "missing" if name not in b else "extra" if name not in a else "same" if a[name][1] == b[name][1] else "DIFFERENT"
        bad += verdict != "same"
        was, now = (a.get(name) or b[name])[0], (b.get(name) or a[name])[0]
        count = per_file.setdefault(was, [0, 0])
        count[0] += 1
        count[1] += verdict == "same"
        insts = sum(1 for ln in (a.get(name) or b[name])[1].splitlines() if ln != ".LBB:")
        print(f"{was if was == now else was + ' -> ' + now}: {verdict:9s} {pretty[name]}  insts={insts}")
    for was, (n, same) in sorted(per_file.items()):
        print(f"{was}: {n} kernels, {same} same, {n - same} not")
    if not src:
        print(f"all sources: {len(set(a) | set(b))} kernels, {bad} not same or duplicate")
    return bad


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--compare":
        sys.exit(1 if compare(*sys.argv[2:5]) else 0)
    tree = sys.argv[1] if len(sys.argv) > 1 else "."
    src = sys.argv[2] if len(sys.argv) > 2 else "lbvh_path.hip"
    for name, r in sorted(resources(tree, src).items()):
        print(f"{name}: " + " ".join(f"{k}={r.get(k, '?')}" for k in ("vgpr", "sgpr", "lds", "scratch", "occ", "insts")))


if __name__ == "__main__":
    main()
