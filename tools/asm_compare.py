#!/usr/bin/env python3
"""asm_compare.py PARENT_DIR HEAD_DIR [--json OUT] -- compare the gfx950 device assembly of two builds, unit by unit and kernel
by kernel.  Each directory holds UNIT.s files made with

    hipcc $(HIPFLAGS) -S --cuda-device-only nbx_UNIT.hip -o - | grep -v __hip_cuid_ > UNIT.s

For every unit: the sha256 prefix of both files.  For every kernel symbol of a unit whose digest differs, the conditions a
refactor must keep -- the same histogram of every non-scalar mnemonic (every mnemonic that does not begin s_, plus s_barrier),
the same LDS bytes, no scratch, the same waves-per-SIMD step -- and, for the record, the scalar and s_waitcnt counts.  Exit
status 1 if a condition fails.  Development harness, not part of the product."""
import collections
import hashlib
import json
import os
import re
import sys


def kernels(text):
    """{symbol: Counter of mnemonics} for every kernel body, {symbol: metadata dict}"""
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)
    hist = {}
    for name in names:
        body = text[text.index("\n%s:" % name):]
        body = body[:body.index(".Lfunc_end")]
        c = collections.Counter()
        for line in body.splitlines():
            m = re.match(r"^\s+([a-z][a-z0-9_]+)(?:\s|$)", line)
            if m and not line.lstrip().startswith("."):
                c[m.group(1)] += 1
        hist[name] = c
    meta = {}
    notes = text[text.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in text else ""
    for block in re.split(r"^  - (?=\.)", notes, flags=re.M)[1:]:
        keys = dict(re.findall(r"^\s*(\.[a-z_]+):\s+(\S+)\s*$", block, re.M))
        if ".name" in keys:
            meta[keys[".name"]] = {k: int(keys.get("." + k, 0)) for k in
                                   ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")}
    return hist, meta


def waves(m):
    """waves per SIMD of a gfx950 kernel: 512 unified registers per lane, allocated in eights"""
    total = (m["vgpr_count"] + 3) // 4 * 4 + m["agpr_count"] if m["agpr_count"] else m["vgpr_count"]
    return min(8, 512 // max(8, (total + 7) // 8 * 8))


def vector_part(c):
    return {k: v for k, v in c.items() if not k.startswith("s_") or k == "s_barrier"}


def main():
    parent, head = sys.argv[1], sys.argv[2]
    out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    ok = True
    report = {}
    for f in sorted(os.listdir(parent)):
        if not f.endswith(".s") or not os.path.exists(os.path.join(head, f)):
            continue
        unit = f[:-2]
        a, b = open(os.path.join(parent, f)).read(), open(os.path.join(head, f)).read()
        da, db = (hashlib.sha256(t.encode()).hexdigest()[:16] for t in (a, b))
        report[unit] = {"parent": da, "head": db, "kernels": {}}
        if da == db:
            print("%-11s %s unchanged" % (unit, da))
            continue
        (ha, ma), (hb, mb) = kernels(a), kernels(b)
        fails = []
        tot = collections.Counter()
        if sorted(ha) != sorted(hb):
            fails.append("kernel symbols differ: %s" % sorted(set(ha) ^ set(hb)))
        for k in sorted(set(ha) & set(hb)):
            same = ha[k] == hb[k] and ma[k] == mb[k]
            row = {"same": same}
            for side, h, m in (("parent", ha[k], ma[k]), ("head", hb[k], mb[k])):
                row[side] = {"scalar": sum(v for n, v in h.items() if n.startswith("s_") and n not in ("s_barrier", "s_waitcnt")),
                             "s_waitcnt": h["s_waitcnt"], "vector": sum(vector_part(h).values()), "vgpr": m["vgpr_count"],
                             "agpr": m["agpr_count"], "lds": m["group_segment_fixed_size"], "waves": waves(m)}
                for key in ("scalar", "s_waitcnt", "vector"):
                    tot[side + key] += row[side][key]
                tot[side + "vgpr_max"] = max(tot[side + "vgpr_max"], m["vgpr_count"] + m["agpr_count"])
            report[unit]["kernels"][k] = row
            if vector_part(ha[k]) != vector_part(hb[k]):
                d = {n: (vector_part(ha[k]).get(n, 0), vector_part(hb[k]).get(n, 0)) for n in set(vector_part(ha[k])) | set(vector_part(hb[k]))
                     if vector_part(ha[k]).get(n, 0) != vector_part(hb[k]).get(n, 0)}
                fails.append("%s: non-scalar histogram %s" % (k, d))
            if ma[k]["group_segment_fixed_size"] != mb[k]["group_segment_fixed_size"]:
                fails.append("%s: LDS %d -> %d" % (k, ma[k]["group_segment_fixed_size"], mb[k]["group_segment_fixed_size"]))
            if mb[k]["private_segment_fixed_size"] != 0:
                fails.append("%s: scratch %d" % (k, mb[k]["private_segment_fixed_size"]))
            if waves(mb[k]) < waves(ma[k]):
                fails.append("%s: waves per SIMD %d -> %d" % (k, waves(ma[k]), waves(mb[k])))
        changed = sum(1 for r in report[unit]["kernels"].values() if not r["same"])
        report[unit]["totals"] = dict(tot)
        report[unit]["fails"] = fails
        print("%-11s %s -> %s  kernels %d (%d differ)  non-scalar %d/%d  scalar %d/%d  s_waitcnt %d/%d  most registers %d/%d  %s"
              % (unit, da, db, len(ha), changed, tot["parentvector"], tot["headvector"], tot["parentscalar"], tot["headscalar"],
                 tot["parents_waitcnt"], tot["heads_waitcnt"], tot["parentvgpr_max"], tot["headvgpr_max"], "FAIL" if fails else "ok"))
        for line in fails:
            print("    " + line)
        ok = ok and not fails
    if out:
        json.dump(report, open(out, "w"), indent=1, sort_keys=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
