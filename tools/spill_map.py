"""Where a step kernel's register spills are: spill stores and reloads per kernel and per source region, from the compiler's own annotations.

One translation unit is compiled to gfx950 assembly with line tables (`hipcc <the build's flags> --cuda-device-only -gline-tables-only -S`, ~2 minutes
for a step-kernel unit).  In that text
  * every spill instruction carries the comment `; 4-byte Folded Spill` (a store to scratch) or `; 4-byte Folded Reload` (a load from it);
  * the `.loc <file> <line> <col>` directive ahead of it names its source line, and the directive's comment the chain of inlined calls the line was
    reached through (`; ./x.h:1850:31 @[ ./x.h:2046:29 @[ ./x.h:2562:25 ] ]`, innermost first);
  * the `amdhsa.kernels` metadata at the end holds, per kernel, the scratch bytes per lane and the VGPR / SGPR spill counts.
Nothing else is read: no instruction is decoded, no register is tracked.

A spill is attributed to a REGION: a function of this repository's sources (a definition that begins in column 0 with `__device__` / `__global__`,
or has a `template <...>` line directly above it).  Of the frames of the inline chain, innermost first, the first one that lies in a STAGE counts
(a function called k_*, as_solve, pgs_sweeps, uhc_step_env or a kernel): a spill inside rcp_newton inside as_solve is as_solve's.  `.loc` lines
with line 0 (compiler-generated code) keep the line before them.  With `--bin N` the stage frame's line is also given, in blocks of N lines.

A spill is IN A LOOP when a backward branch (a branch, short or long, to a label defined above it in the text) encloses it: "in loop" counts those, the
others execute once per kernel.  That is a reading of the text's order, not of the control-flow graph -- good enough to tell "ahead of the substep loop"
from "every substep".

    python tools/spill_map.py uhc_k_fast_dense.hip [--kernel SUBSTR] [--bin 50] [--flags "-DX ..."]     compile, then print
    python tools/spill_map.py --asm unit.s [--kernel SUBSTR] [--bin 50]                                  print from assembly that is already there
"""
import bisect
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uhc_amd", "csrc")

FILE_DIR = re.compile(r'^\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?')
LOC = re.compile(r"^\s*\.loc\s+(\d+)\s+(\d+)\s+(\d+)[^;]*(?:;(.*))?$")
FRAME = re.compile(r"([^\s\[\]@;]+):(\d+):\d+")
LABEL = re.compile(r"^([.\w$@]+):")
BRANCH = re.compile(r"^\s*s_c?branch\w*\s+([.\w$@]+)")
LONG_BRANCH = re.compile(r"^\s*s_add_u32\s.*\(([.\w$@]+)-\.Lpost_getpc\d+\)")  # a branch beyond the short form's reach: s_getpc_b64 / s_add_u32 / s_addc_u32 / s_setpc_b64
SPILL = re.compile(r";\s*(\d+)-byte Folded (Spill|Reload)")
KERNEL_BEGIN = re.compile(r"^\s*\.type\s+([.\w$@]+),@function")
KERNEL_END = re.compile(r"^\s*\.size\s+([.\w$@]+),")
META_ITEM = re.compile(r"^(\s*)(-\s+)?\.(\w+):\s+(.*\S)\s*$")
STAGE = re.compile(r"^(k_\w+|as_solve|pgs_sweeps|uhc_step_env|uhc_step_kernel|uhc_step_queue_kernel)$")


def parse_asm(text):
    """-> (kernels, meta).  kernels: {symbol: [spill, ...]} in text order, a spill = dict(kind 'store' | 'reload', bytes, frames [(file, line), ...]
    innermost first, in_loop); meta: {symbol: {key: value string}} of the amdhsa.kernels notes."""
    files = {}
    kernels = collections.OrderedDict()
    cur = None          # symbol of the function being read
    frames = []
    labels = {}         # label -> index of its line
    events = []         # (index, kind, bytes, frames) of the function's spills
    branches = []       # (index, target)
    items = []
    in_meta, item, item_indent = False, None, None

    def close():
        nonlocal events, branches, labels
        if cur is None:
            return
        loops = [(labels[t], i) for i, t in branches if t in labels and labels[t] <= i]  # backward branches: [label, branch]
        kernels[cur] = [{"kind": kind, "bytes": nbytes, "frames": fr, "in_loop": any(a <= i <= b for a, b in loops)} for i, kind, nbytes, fr in events]
        events, branches, labels = [], [], {}

    for idx, raw in enumerate(text.splitlines()):
        m = FILE_DIR.match(raw)
        if m:
            files[int(m.group(1))] = os.path.join(m.group(2), m.group(3)) if m.group(3) else m.group(2)
            continue
        if raw.startswith("amdhsa.kernels:"):
            in_meta = True
            continue
        if in_meta:
            if raw.startswith("amdhsa.") or raw.strip() in ("...", "---"):
                in_meta = False
                continue
            m = META_ITEM.match(raw)
            if m:
                indent = len(m.group(1))
                if m.group(2) and (item_indent is None or indent <= item_indent):  # a new item of the kernels list (nested lists are indented further)
                    item, item_indent = {}, indent
                    items.append(item)
                if item is not None and indent <= item_indent + 2:
                    item[m.group(3)] = m.group(4).strip("'\"")
            continue
        m = KERNEL_BEGIN.match(raw)
        if m:
            close()
            cur, frames = m.group(1), []
            continue
        if cur is None:
            continue
        m = KERNEL_END.match(raw)
        if m and m.group(1) == cur:
            close()
            cur = None
            continue
        m = LOC.match(raw)
        if m:
            if int(m.group(2)) != 0:
                chain = FRAME.findall(m.group(4) or "")
                frames = [(f, int(l)) for f, l in chain] if chain else [(files.get(int(m.group(1)), "?"), int(m.group(2)))]
            continue
        m = LABEL.match(raw)
        if m:
            labels[m.group(1)] = idx
            continue
        m = BRANCH.match(raw) or LONG_BRANCH.match(raw)
        if m:
            branches.append((idx, m.group(1)))
            continue
        m = SPILL.search(raw)
        if m:
            events.append((idx, "store" if m.group(2) == "Spill" else "reload", int(m.group(1)), frames))
    close()
    return kernels, {it["name"]: it for it in items if "name" in it}


FUNC = re.compile(r"^(?:static\s+|inline\s+)*(?:__device__|__global__)\b.*?\b([A-Za-z_]\w*)\s*\(")


def regions_of(source_text):
    """[(first line, name)] of the functions a source file defines in column 0, ascending."""
    out = []
    lines = source_text.splitlines()
    for n, l in enumerate(lines, 1):
        m = FUNC.match(re.sub(r"__launch_bounds__\([^)]*\)", "", l))
        if m and not l.rstrip().endswith(";"):
            out.append((n - 1 if n >= 2 and lines[n - 2].startswith("template") else n, m.group(1)))
    return out


def region_name(regions, line):
    k = bisect.bisect_right([r[0] for r in regions], line) - 1
    return regions[k][1] if k >= 0 else "(head)"


def stage_of(frames, regions_for):
    """(file, region, line) of the frame a spill is attributed to.  regions_for(file) -> [(first line, name)] or [] (a file that is not ours)."""
    named = []
    for f, line in frames:
        regs = regions_for(f)
        if regs:
            named.append((os.path.basename(f), region_name(regs, line), line))
    for n in named:
        if STAGE.match(n[1]):
            return n
    if named:
        return named[0]
    f, line = frames[0] if frames else ("?", 0)
    return (os.path.basename(f), "l. %d" % line, line)


def demangle(sym):
    for tool in ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            r = subprocess.run([tool, sym], capture_output=True, text=True)
        except OSError:
            continue
        if r.returncode == 0 and r.stdout.strip():
            return re.sub(r"\(.*", "", r.stdout.strip()).replace("void ", "")
    return sym


def report(kernels, meta, want=None, bin_lines=0, read_source=None, name_of=demangle):
    """The printed table as a list of lines.  read_source(path) -> text or None (regions by function need the source)."""
    out = []
    cache = {}

    def regions_for(f):
        if f not in cache:
            txt = read_source(f) if read_source else None
            cache[f] = regions_of(txt) if txt else []
        return cache[f]

    for sym, spills in kernels.items():
        name = name_of(sym)
        if want and want not in name and want not in sym:
            continue
        m = meta.get(sym, {})
        if not spills and not m:
            continue
        out.append("%s: scratch %s B/lane, VGPR spills %s, SGPR spills %s, vgpr %s agpr %s sgpr %s" % (
            name, m.get("private_segment_fixed_size", "?"), m.get("vgpr_spill_count", "?"), m.get("sgpr_spill_count", "?"),
            m.get("vgpr_count", "?"), m.get("agpr_count", "?"), m.get("sgpr_count", "?")))
        tab = {}
        for s in spills:
            f, region, line = stage_of(s["frames"], regions_for)
            lo = (line // bin_lines) * bin_lines if bin_lines else 0
            row = tab.setdefault((f, region, lo), [0, 0, 0, 0])
            row[(0 if s["kind"] == "store" else 2) + (1 if s["in_loop"] else 0)] += 1
        out.append("    %-24s %-24s %-14s %8s %8s %8s %8s" % ("file", "region", "lines", "stores", "in loop", "reloads", "in loop"))
        tot = [0, 0, 0, 0]
        for key in sorted(tab):
            r = tab[key]
            out.append("    %-24s %-24s %-14s %8d %8d %8d %8d" % (key[0][:24], key[1][:24], "%d-%d" % (key[2], key[2] + bin_lines - 1) if bin_lines else "",
                                                                 r[0] + r[1], r[1], r[2] + r[3], r[3]))
            tot = [a + b for a, b in zip(tot, r)]
        out.append("    %-24s %-24s %-14s %8d %8d %8d %8d" % ("total", "", "", tot[0] + tot[1], tot[1], tot[2] + tot[3], tot[3]))
    return out


def compile_unit(src, extra_flags, out):
    sys.path.insert(0, ROOT)
    from __graft_entry__ import _hipcc, unit_flags
    subprocess.check_call([_hipcc()] + unit_flags(extra_flags, os.path.basename(src)) + ["--cuda-device-only", "-gline-tables-only", "-S", src, "-o", out], cwd=CSRC)


def _read(path):
    for p in (path, os.path.join(CSRC, path), os.path.join(CSRC, os.path.basename(path))):
        if os.path.isfile(p) and os.path.realpath(p).startswith(os.path.realpath(ROOT) + os.sep):
            return open(p, errors="replace").read()
    return None


def main(argv):
    want, bin_lines, asm, flags, src = None, 0, None, [], None
    a = list(argv)
    while a:
        x = a.pop(0)
        if x == "--kernel":
            want = a.pop(0)
        elif x == "--bin":
            bin_lines = int(a.pop(0))
        elif x == "--asm":
            asm = a.pop(0)
        elif x == "--flags":
            flags = a.pop(0).split()
        else:
            src = x
    if asm is None:
        if src is None:
            print(__doc__)
            return 2
        asm = os.path.join(tempfile.mkdtemp(), os.path.basename(src) + ".s")
        compile_unit(src, flags, asm)
    kernels, meta = parse_asm(open(asm, errors="replace").read())
    print("# tools/spill_map.py %s" % " ".join(os.path.basename(x) if os.sep in x else x for x in argv))
    print("\n".join(report(kernels, meta, want, bin_lines, _read)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
