"""Compare two device-only assembly listings (hipcc --cuda-device-only -S) kernel by kernel.

python cmp_asm.py parent.s new.s [--list]

Per kernel symbol: the body with comments dropped and basic-block labels renumbered in order of appearance, and the
resource lines the compiler prints after it (SGPRs, VGPRs, AGPRs, scratch, occupancy, static LDS).  Prints the
conditions a refactor of kernels is held to (profiles/conv_epilogue/README.md) and, per kernel family, how the
differing bodies differ: only in register numbers (every other operand, immediate and offset equal), the same
instructions in another order, or by instruction count.
"""
import collections
import re
import subprocess
import sys

INFO = {"TotalNumSgprs": "sgpr", "NumVgprs": "vgpr", "NumAgprs": "agpr", "ScratchSize": "scratch", "Occupancy": "occ",
        "LDSByteSize": "lds"}


def parse(path):
    kernels, cur, body, info = {}, None, [], None
    syms = set()
    lines = open(path).read().splitlines()
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            syms.add(m.group(1))
    for ln in lines:
        m = re.match(r"^(\S+):\s*(;.*)?$", ln)
        if m and m.group(1) in syms and cur is None:
            cur, body, info = m.group(1), [], {}
            continue
        if cur is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", ln):
            kernels[cur] = {"body": body, "info": info}
            body = None
            continue
        if body is not None:
            code = ln.split(";", 1)[0].rstrip()
            if code.strip():
                body.append(code.strip())
        else:
            m = re.match(r"^;\s*(\w+):\s*(\d+)", ln)
            if m and m.group(1) in INFO:
                info[INFO[m.group(1)]] = int(m.group(2))
            if "Occupancy" in ln:
                cur = None
    return kernels


def renumber(body):
    names = {}
    def sub(m):
        return names.setdefault(m.group(0), ".L%d" % len(names))
    return [re.sub(r"\.LBB\d+_\d+", sub, ln) for ln in body]


def insns(body):
    return [ln for ln in body if not ln.startswith(".") and not ln.endswith(":")]


def noregs(body):
    """register numbers replaced (v12, s[4:5], a3 -> v, s, a); immediates, offsets, waitcnt values and labels stay"""
    return [re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1", ln) for ln in body]


def family(dem):
    m = re.search(r"can::(\w+)", dem)
    return m.group(1) if m else dem


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    show = "--list" in sys.argv
    names = sorted(set(a) | set(b))
    dem = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), text=True,
                                         capture_output=True).stdout.splitlines()))
    print("symbols: parent %d, new %d, only parent %d, only new %d" % (len(a), len(b), len(set(a) - set(b)),
                                                                       len(set(b) - set(a))))
    same = 0
    worse = collections.defaultdict(list)
    fam = collections.defaultdict(lambda: collections.Counter())
    regs = []
    for k in sorted(set(a) & set(b)):
        ia, ib = a[k]["info"], b[k]["info"]
        if ib["scratch"] > ia["scratch"]: worse["scratch"].append(k)
        if ib["occ"] < ia["occ"]: worse["occupancy"].append(k)
        if ib["lds"] != ia["lds"]: worse["lds"].append(k)
        if (ia["vgpr"], ia["agpr"], ia["sgpr"]) != (ib["vgpr"], ib["agpr"], ib["sgpr"]):
            regs.append((dem[k], ia, ib))
        ba, bb = renumber(a[k]["body"]), renumber(b[k]["body"])
        f = family(dem[k])
        if ba == bb:
            same += 1
            fam[f]["identical"] += 1
            continue
        na, nb = insns(ba), insns(bb)
        ma, mb = [x.split()[0] for x in na], [x.split()[0] for x in nb]
        if noregs(ba) == noregs(bb):
            kind = "register numbers only"
        elif sorted(noregs(na)) == sorted(noregs(nb)):
            kind = "same instructions (operands but register numbers included), order differs"
        elif ma == mb:
            kind = "same mnemonic sequence, operands differ"
        elif sorted(ma) == sorted(mb):
            kind = "same mnemonics, order differs"
        else:
            kind = "instruction count %+d" % (len(nb) - len(na)) if len(nb) != len(na) else "same count, other instructions"
        fam[f][kind] += 1
        if show:
            print("  %-60s %s (%d -> %d)" % (dem[k][:150], kind, len(na), len(nb)))
    print("identical bodies: %d of %d" % (same, len(set(a) & set(b))))
    for w in ("scratch", "occupancy", "lds"):
        print("%s worse / changed: %d" % (w, len(worse[w])), [dem[k] for k in worse[w]][:20])
    print("scratch at parent:", dict(collections.Counter(v["info"]["scratch"] for v in a.values())))
    for f, c in sorted(fam.items()):
        print("%-28s %s" % (f, dict(c)))
    print("register counts that differ (sgpr / vgpr / agpr, parent -> new): %d" % len(regs))
    for d, ia, ib in regs:
        print("  %s: %d / %d / %d -> %d / %d / %d, occ %d -> %d" % (d[:160], ia["sgpr"], ia["vgpr"], ia["agpr"], ib["sgpr"],
                                                                  ib["vgpr"], ib["agpr"], ia["occ"], ib["occ"]))


main()
