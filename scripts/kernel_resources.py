#!/usr/bin/env python3
"""Per-kernel register/LDS/scratch figures and instruction counts (CPU only).

  python scripts/kernel_resources.py deepconsensus_amd/ops/hip/fused_ffn_v5.hip

Cross-compiles each .hip file device-only for gfx950 with DC_SAN_MAIN set
(no torch headers) and reads the code-object metadata and the assembly.
A kernel template is instantiated for every `name<N>` the file spells out.
"""
import os
import re
import subprocess
import sys
import tempfile

META = (".vgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".private_segment_fixed_size", ".group_segment_fixed_size")
INSTS = ("v_mfma", "ds_read_b128", "global_load_lds", "s_barrier")


def kernels_of(src):
    names = []
    pat = (r"(template\s*<[^>]*>\s*)?__global__\s+"
           r"(?:__launch_bounds__\([^)]*\)\s*)?void\s+(\w+)\s*\(")
    for tmpl, name in re.findall(pat, src):
        if tmpl:
            names += sorted(set(re.findall(rf"\b{name}<\d+>", src)))
        else:
            names.append(name)
    return names


def report(path):
    path = os.path.abspath(path)
    names = kernels_of(open(path).read())
    with tempfile.TemporaryDirectory() as tmp:
        tu, asm = os.path.join(tmp, "tu.hip"), os.path.join(tmp, "tu.s")
        keep = ", ".join(f"(void*)&{n}" for n in names)
        with open(tu, "w") as f:
            f.write(f'#include <hip/hip_runtime.h>\n#include "{path}"\n'
                    f"void* dc_keep[] = {{{keep}}};\n")
        subprocess.run(
            ["hipcc", "-DDC_SAN_MAIN=1", "-O3", "--offload-arch=gfx950",
             "--cuda-device-only", "-std=c++17", "-S", tu, "-o", asm],
            check=True)
        text = open(asm).read()
    print(os.path.basename(path))
    # One YAML list item per kernel under amdhsa.kernels, keys sorted.
    for meta in re.split(r"^\s+- \.agpr_count:", text, flags=re.M)[1:]:
        sym = re.search(r"^\s+\.name:\s+(\S+)$", meta, re.M).group(1)
        body = re.search(rf"^{sym}:.*?^\s+\.size\s+{sym},", text,
                         re.M | re.S).group(0)
        name = subprocess.run(["c++filt", "-p", sym], capture_output=True,
                              text=True).stdout.strip() or sym
        name = name.replace("(anonymous namespace)::", "").replace("void ", "")
        cols = [k + "=" + re.search(re.escape(k) + r":\s+(\d+)", meta).group(1)
                for k in META]
        cols += [i + "=" + str(len(re.findall(r"^\s+" + i, body, re.M)))
                 for i in INSTS]
        print(f"  {name}: " + " ".join(cols))


if __name__ == "__main__":
    for p in sys.argv[1:]:
        report(p)
