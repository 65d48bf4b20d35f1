"""The one `--resources` of the tools: registers, LDS and scratch of every kernel of a file of rpvg_amd/csrc from hipcc's resource
remarks (gfx950).  Cross-compiles; needs no GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_REMARK = re.compile(r"remark: (?:\s*)(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|"
                     r"Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\S+)")


def resource_usage(source_file, out, header_note="", width=34, spills=False, footer=()):
    """Writes one line per kernel of rpvg_amd/csrc/<source_file> (hipcub's own kernels left out) to `out` and prints it.  header_note
    goes behind the first line, `footer` lines behind the table; spills adds the two spill columns.  A kernel with scratch is an error."""
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(ROOT, "rpvg_amd", "csrc", source_file),
           "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    kernels, current = [], None
    for line in text.splitlines():
        m = _REMARK.search(line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            current = {"name": m.group(2)}
            kernels.append(current)
        elif current is not None:
            current[m.group(1)] = m.group(2)
    columns = [("VGPRs", "VGPRs", 7), ("SGPRs", "TotalSGPRs", 7), ("LDS B", "LDS Size [bytes/block]", 8), ("scratch B/lane", "ScratchSize [bytes/lane]", 16),
               ("waves/SIMD", "Occupancy [waves/SIMD]", 12)]
    if spills:
        columns += [("SGPR spills", "SGPRs Spill", 13), ("VGPR spills", "VGPRs Spill", 13)]
    lines = [f"{source_file}, hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage{header_note}",
             f"{'kernel':<{width}}" + "".join(f"{title:>{w}}" for title, _, w in columns)]
    for k in kernels:
        name = subprocess.run(["c++filt", k["name"]], capture_output=True, text=True).stdout.strip() or k["name"]
        if "hipcub" in name or "rocprim" in name or "Kernel" not in name:
            continue
        short = re.sub(r"^.*?(\w+Kernel)(<[^(]*>)?\(.*$", r"\1\2", name).replace("(anonymous namespace)::", "")
        lines.append(f"{short:<{width}}" + "".join(f"{k.get(key, '?'):>{w}}" for _, key, w in columns))
        assert k.get("ScratchSize [bytes/lane]") == "0", f"{short} uses scratch"
    lines += list(footer)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
