"""Device code of two source trees, compared per kernel symbol: is a refactor of csrc/ the same machine code?
   python tools/device_asm_diff.py --parent HEAD~ [-DFLAG ...]      the working tree against a git revision (exported into a temporary directory)
   python tools/device_asm_diff.py TREE_A TREE_B [-DFLAG ...]       two checked-out trees
Every .hip unit of build.UNITS is compiled on both sides with build.FLAGS + `-S --cuda-device-only` (+ the -D flags given, on both
sides), the assembly is split per symbol -- a function's text from `.type NAME,@function` to `.size NAME`, its kernel descriptor and its
resource `.set` lines; a data object (constant tables) likewise; all other directives, sorted, as one pseudo-symbol -- comments are
dropped and local labels lose the function index they carry (.LBB12_3 -> .LBB_3: the index moves with emission order, not with the
code).  The metadata note is not compared: it restates the descriptors.  Printed per unit: function symbols, descriptors, instruction
lines, and every symbol whose text differs (first differing lines) or that one side alone has.  Exit status 1 on any difference.
Text is split, normalised and compared; nothing in it is interpreted."""
import argparse
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LABEL = re.compile(r"(\.L[A-Za-z_]+?)\d+(_\d+)?\b")
_CUID = re.compile(r"__hip_cuid_[0-9a-f]+")
_TYPE = re.compile(r"^\s*\.type\s+(\S+),@(function|object)")
_SIZE = re.compile(r"^\s*\.size\s+(\S+),")
_DESC = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
_SET = re.compile(r"^\s*\.set\s+(\S+)\.[a-z_]+,")
REST = "(rest of the unit)"


def normalise(line):
    """One assembly line without its comment (a ';' outside double quotes starts one), trailing blanks, the function index of local
    labels and the hash in the compilation unit's id symbol; '' if nothing is left."""
    quoted = False
    for i, c in enumerate(line):
        if c == '"' and (i == 0 or line[i - 1] != "\\"):
            quoted = not quoted
        elif c == ";" and not quoted:
            line = line[:i]
            break
    return _CUID.sub("__hip_cuid", _LABEL.sub(lambda m: m.group(1) + (m.group(2) or ""), line.rstrip()))


def split_symbols(asm):
    """({symbol: normalised lines}, number of function symbols, number of kernel descriptors) of one assembly text.  A function or data
    object is its text from `.type NAME,@function|@object` to `.size NAME`; a function also owns its kernel descriptor and its resource
    `.set` lines.  Every other line outside the metadata note (section switches, visibility, ident) goes, sorted, into the pseudo-symbol
    REST, so that nothing of the unit is left uncompared and the order of emission does not count."""
    syms, cur, in_desc, in_meta, n_func, n_desc = {REST: []}, None, None, False, 0, 0
    for raw in asm.split("\n"):
        line = normalise(raw)
        if not line:
            continue
        if line.strip() in (".amdgpu_metadata", ".end_amdgpu_metadata"):      # restates the descriptors, with the kernels in emission order
            in_meta = line.strip() == ".amdgpu_metadata"
            continue
        if in_meta:
            continue
        m = _TYPE.match(line)
        if m:
            cur = m.group(1)
            syms.setdefault(cur, [])
            n_func += m.group(2) == "function"
        m = _DESC.match(line)
        if m:
            in_desc = m.group(1)
            n_desc += 1
        m = _SET.match(line)
        if in_desc is not None:
            syms.setdefault(in_desc, []).append(line)
            if line.strip() == ".end_amdhsa_kernel":
                in_desc = None
        elif m and m.group(1) in syms:
            syms[m.group(1)].append(line)
        elif cur is not None:
            syms[cur].append(line)
            m = _SIZE.match(line)
            if m and m.group(1) == cur:
                cur = None
        else:
            syms[REST].append(line)
    syms[REST].sort()
    return syms, n_func, n_desc


def is_instruction(line):
    s = line.strip()
    return not (s.startswith(".") or s.endswith(":"))


def compare(syms_a, syms_b):
    """[(symbol, what)] for every symbol that differs: what = 'only in A', 'only in B' or the first differing lines as a unified diff."""
    out = []
    for name in sorted(set(syms_a) | set(syms_b)):
        if name not in syms_b:
            out.append((name, "only in A"))
        elif name not in syms_a:
            out.append((name, "only in B"))
        elif syms_a[name] != syms_b[name]:
            d = list(difflib.unified_diff(syms_a[name], syms_b[name], "A", "B", n=1, lineterm=""))
            out.append((name, "\n".join(d[:40] + (["... (%d more diff lines)" % (len(d) - 40)] if len(d) > 40 else []))))
    return out


def device_asm(cmd, src, out):
    r = subprocess.run(cmd + ["-S", "--cuda-device-only", "-o", out, src], stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s does not compile:\n%s" % (src, "\n".join(r.stderr.split("\n")[:30])))
    with open(out) as f:
        return f.read()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("trees", nargs="*", help="two source trees A B (or none with --parent)")
    ap.add_argument("--parent", metavar="REV", help="A = this git revision, B = the working tree")
    ap.add_argument("-D", dest="defines", action="append", default=[], metavar="NAME[=VALUE]", help="extra definition, applied to both sides")
    ap.add_argument("-j", type=int, default=4, help="compilations at a time")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "rgbd360_amd"))
    import build
    units = [u for u in build.UNITS if u.endswith(".hip")]
    defines = ["-D" + d for d in a.defines]
    cmd = [build.hipcc()] + [f for f in build.FLAGS if f not in ("-shared", "-pthread")] + defines
    with tempfile.TemporaryDirectory(prefix="device_asm_diff_") as tmp:
        if a.parent:
            if a.trees:
                ap.error("--parent takes no trees")
            tree_a, tree_b = os.path.join(tmp, "parent"), ROOT
            os.makedirs(tree_a)
            tar = subprocess.run(["git", "-C", ROOT, "archive", a.parent, "rgbd360_amd/csrc", "include"], check=True, stdout=subprocess.PIPE).stdout
            subprocess.run(["tar", "-x", "-C", tree_a], input=tar, check=True)
        elif len(a.trees) == 2:
            tree_a, tree_b = (os.path.abspath(t) for t in a.trees)
        else:
            ap.error("give two trees or --parent REV")
        with concurrent.futures.ThreadPoolExecutor(a.j) as pool:
            jobs = {(u, side): pool.submit(device_asm, cmd, os.path.join(tree, "rgbd360_amd", "csrc", u), os.path.join(tmp, side + "_" + u + ".s"))
                    for u in units for side, tree in (("A", tree_a), ("B", tree_b))}
            texts = {k: j.result() for k, j in jobs.items()}
    print("A = %s, B = %s, flags: build.FLAGS %s" % (a.parent or tree_a, tree_b, " ".join(defines)))
    n_diff = 0
    for u in units:
        (sa, fa, da), (sb, fb, db) = split_symbols(texts[(u, "A")]), split_symbols(texts[(u, "B")])
        ia, ib = (sum(is_instruction(l) for n, ls in s.items() if n != REST for l in ls) for s in (sa, sb))
        diffs = compare(sa, sb)
        n_diff += len(diffs) + (da != db) + (fa != fb)
        print("%s: symbols %d / %d, descriptors %d / %d, instruction lines %d / %d, differing symbols %d" % (u, fa, fb, da, db, ia, ib, len(diffs)))
        for name, what in diffs:
            print("  %s: %s" % (name, what))
    print("IDENTICAL" if n_diff == 0 else "DIFFERENT")
    return 1 if n_diff else 0


if __name__ == "__main__":
    sys.exit(main())
