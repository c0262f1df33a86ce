#!/usr/bin/env python3
"""Register / LDS / spill numbers of every kernel of the library, from hipcc -Rpass-analysis=kernel-resource-usage
(runs without a GPU).  usage: kernel_resources.py [substring ...] [-- extra hipcc flags]
The batch solves and their guards: `kernel_resources.py batch ell matching sparse_outside` (k_dense_* / k_sparse_batch_* /
k_ell_* / k_matching_batch*, the outside modes k_dense_outside_solve<T, Lay> / k_ell_outside_solve<I, V> and
k_sparse_outside_solve<Src>; the check pass of both modes is k_dense_batch_check<T, Lay, Out>, Lay being DenseContig or
DenseView<Fin>, k_sparse_batch_check<Src, Out>, Src being SparsePacked or SparseView<I, V>, and
k_ell_batch_check<I, V, Out>).
With --code-size the device code is compiled once more on its own and every line ends in code=<bytes>, the size of the
kernel's symbol in the gfx950 code object (the comparisons of DESIGN 4.20, 4.21 and 4.22:
`kernel_resources.py --code-size dense matching_batch`, `kernel_resources.py --code-size ell sparse matching_batch`)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sslap_amd import build  # noqa: E402

args = sys.argv[1:]
code_size = "--code-size" in args
args = [a for a in args if a != "--code-size"]
extra = []
if "--" in args:
    k = args.index("--")
    args, extra = args[:k], args[k + 1:]
cmd = [build.hipcc()] + build.FLAGS + extra + ["-Rpass-analysis=kernel-resource-usage", os.path.join(build.CSRC, "misslap.hip"),
                                                "-o", "/tmp/_kernel_resources.so"]
txt = subprocess.run(cmd, cwd=build.CSRC, capture_output=True, text=True).stderr
code = {}
if code_size:  # mangled kernel name -> bytes, from the symbol table of the unbundled device object
    llvm = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc()))), "lib", "llvm", "bin")
    dev, elf = "/tmp/_kernel_resources_dev.o", "/tmp/_kernel_resources_gfx950.elf"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([build.hipcc()] + flags + extra + ["--cuda-device-only", "-c", os.path.join(build.CSRC, "misslap.hip"),
                                                            "-o", dev], cwd=build.CSRC)
    subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + dev,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + elf])
    for line in subprocess.run([os.path.join(llvm, "llvm-readelf"), "-sW", elf], capture_output=True, text=True).stdout.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC":
            code[f[7]] = int(f[2])
KEYS = (("sgpr", r"TotalSGPRs"), ("vgpr", r"VGPRs"), ("scratch", r"ScratchSize \[bytes/lane\]"),
        ("occ", r"Occupancy \[waves/SIMD\]"), ("sgpr_spill", r"SGPRs Spill"), ("vgpr_spill", r"VGPRs Spill"),
        ("lds", r"LDS Size \[bytes/block\]"))
for b in re.split(r"remark: Function Name: ", txt)[1:]:
    mangled = b.split()[0]
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
    name = re.sub(r"^void misslap::", "", name)
    depth = 0  # the name without its parameter list (a template argument may hold parentheses of its own)
    for k in range(len(name) - 1, -1, -1):
        depth += (name[k] == ")") - (name[k] == "(")
        if depth == 0:
            name = name[:k] if name[k] == "(" else name
            break
    if args and not any(a in name for a in args):
        continue
    vals = []
    for label, key in KEYS:
        m = re.search(key + r": (\d+)", b)
        vals.append(f"{label}={m.group(1) if m else '?'}")
    if code_size:
        vals.append(f"code={code.get(mangled, '?')}")
    print(f"{name[:88]:88s} " + " ".join(vals))
