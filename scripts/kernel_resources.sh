#!/bin/bash
# Resource usage (VGPRs, spills, scratch, LDS, occupancy) of every kernel of one translation unit, from the compiler's own remarks,
# and what its scalar spills cost in the instruction stream, counted in the compiler's assembly: the kernel's .sgpr_spill_count, its
# v_readlane_b32 (reloads) and v_writelane_b32 (spills) and the vector instructions (v_*, ds_*, global_*, flat_*, buffer_*) they stand among:
#   scripts/kernel_resources.sh kmu_sketch [filter]
cd "$(dirname "$0")/../kmerutils_amd/csrc" || exit 1
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wno-unused-function $KMU_BUILD_DEFS"
ASM=$(mktemp) || exit 1
trap 'rm -f "$ASM"' EXIT
/opt/rocm/bin/hipcc $FLAGS --cuda-device-only -S "$1.hip" -o "$ASM" 2>/dev/null || exit 1
/opt/rocm/bin/hipcc $FLAGS -Rpass-analysis=kernel-resource-usage -c "$1.hip" -o /dev/null 2>&1 | python3 -c '
import re, sys, subprocess
cur = None; rows = []
for line in sys.stdin:
    m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
    if not m: continue
    t = m.group(1).strip()
    if t.startswith("Function Name:"):
        cur = {"name": t.split(":", 1)[1].strip()}; rows.append(cur)
    elif cur is not None and ":" in t:
        k, v = t.rsplit(":", 1); cur[k.strip()] = v.strip()
# the assembly: lane moves and vector instructions between a kernel label and its s_endpgm, the spill count of its metadata
lanes = {}; name = None
for line in open(sys.argv[2]):
    t = line.split()
    if not t: continue
    if not line[0].isspace() and t[0].endswith(":") and not t[0].startswith("."):
        name = t[0][:-1]; lanes[name] = [0, 0, 0, None]
    elif name and line[0].isspace():
        op = t[0]
        if op == "v_readlane_b32": lanes[name][0] += 1
        elif op == "v_writelane_b32": lanes[name][1] += 1
        if op.startswith(("v_", "ds_", "global_", "flat_", "buffer_")): lanes[name][2] += 1
        if op == "s_endpgm": name = None
    m = re.match(r"\s+\.name:\s+(\S+)", line)
    if m: meta = m.group(1)
    m = re.match(r"\s+\.sgpr_spill_count:\s+(\d+)", line)
    if m: sp = int(m.group(1))
    if re.match(r"\s+\.vgpr_spill_count:", line) and meta in lanes: lanes[meta][3] = sp  # (the last of a kernel: .name and .sgpr_spill_count stand in front of it)
flt = sys.argv[1] if len(sys.argv) > 1 else ""
for r in rows:
    try: name = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-cxxfilt", r["name"]], capture_output=True, text=True).stdout.strip()
    except Exception: name = r["name"]
    name = re.sub(r"\(.*", "", name)
    if flt and flt not in name: continue
    ln = lanes.get(r["name"], [None] * 4)
    print("%-70s vgpr %3s agpr %3s sgpr %3s  spill v %3s s %3s  scratch %4s B  lds %6s B  occupancy %s | .sgpr_spill_count %s  v_readlane_b32 %s  v_writelane_b32 %s  of %s vector instructions" % (
        name[:70], r.get("VGPRs"), r.get("AGPRs"), r.get("TotalSGPRs"), r.get("VGPRs Spill", r.get("VGPR Spill")), r.get("SGPRs Spill", r.get("SGPR Spill")),
        r.get("ScratchSize [bytes/lane]"), r.get("LDS Size [bytes/block]"), r.get("Occupancy [waves/SIMD]"), ln[3], ln[0], ln[1], ln[2]))
' "$2" "$ASM"
