"""Per kernel of two device-only code objects: instruction bytes (llvm-objdump -d, split at the
kernel symbols; the pc-relative literal after s_getpc_b64 left out) and the notes metadata."""
import hashlib
import re
import subprocess
import sys

LLVM = "/opt/rocm/llvm/bin/"


def kernels(co):
    dis = subprocess.run([LLVM + "llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout
    out, cur, skip = {}, None, 0
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            skip = 0
            continue
        if cur is None or "//" not in line:
            continue
        text, enc = line.split("//", 1)
        words = enc.split(":", 1)[1].split()
        mnem = text.split()[0]
        if skip:  # the s_add_u32 / s_addc_u32 after s_getpc_b64 carry the pc-relative literal
            if mnem.startswith("s_add_u32") or mnem.startswith("s_addc_u32"):
                words = words[:1]
            skip -= 1
        if mnem == "s_getpc_b64":
            skip = 2
        out[cur].append((mnem, tuple(words)))
    return out


def notes(co):
    txt = subprocess.run([LLVM + "llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    res = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", txt)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        f = {k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)
             for k in ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count",
                       "private_segment_fixed_size", "group_segment_fixed_size", "max_flat_workgroup_size",
                       "kernarg_segment_size", "wavefront_size")}
        f["agpr_count"] = blk.split()[0]
        res[name] = f
    return res


def table(co):
    k, n = kernels(co), notes(co)
    rows = {}
    for name, meta in n.items():
        ins = k[name]
        h = hashlib.sha256(repr(ins).encode()).hexdigest()[:16]
        rows[name] = (len(ins), h, meta)
    return rows


def main(a, b, out_a, out_b):
    ta, tb = table(a), table(b)
    for t, path in ((ta, out_a), (tb, out_b)):
        with open(path, "w") as f:
            f.write("# kernel  instructions  sha256(instruction bytes)[:16]  vgpr sgpr sgpr_spill vgpr_spill scratch lds\n")
            for name in sorted(t):
                n, h, m = t[name]
                demangled = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
                f.write(f"{name}  {demangled}  {n}  {h}  {m['vgpr_count']} {m['sgpr_count']} {m['sgpr_spill_count']} "
                        f"{m['vgpr_spill_count']} {m['private_segment_fixed_size']} {m['group_segment_fixed_size']}\n")
    print("parent", len(ta), "branch", len(tb))
    print("only parent:", sorted(set(ta) - set(tb)))
    print("only branch:", sorted(set(tb) - set(ta)))
    diff = [k for k in ta if k in tb and ta[k] != tb[k]]
    print("differing:", diff)
    return 0 if not diff and set(ta) == set(tb) else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:5]))
