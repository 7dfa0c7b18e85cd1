"""Compare two gfx950 assembly files (hipcc --save-temps: *-gfx950.s) function by function: instruction lines only, comments and
debug / alignment directives dropped, labels renumbered in order of appearance, mangled names inside instructions replaced.  python tools/isa_diff.py old.s new.s
[SED-STYLE-RENAME ...]   e.g.  's/ILi(\\d+)ELb1EE/ILi\\1EE/'  maps the function names of old.s onto those of new.s.  Exit status 1 on a difference."""
import re, sys
SKIP = re.compile(r"\s*\.(loc|file|cfi\w*|p2align|globl|protected|section|text|weak|hidden)\b")


def functions(path, renames):
    out, name, labels = {}, None, {}
    for line in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name = m.group(1)
            for a, b in renames: name = re.sub(a, b, name)
            out[name] = []; labels = {}; continue
        if name is None: continue
        if re.match(r"\s*\.size\s", line): name = None; continue
        line = line.split(";")[0].strip()
        if not line or SKIP.match(line) or line.endswith(":") and line.startswith(("_Z", ".Lfunc")): continue
        line = re.sub(r"_Z\w+", "SYM", line)
        out[name].append(re.sub(r"\.L\w+", lambda m: ".L%d" % labels.setdefault(m.group(0), len(labels)), line))   # in order of appearance
    return out


renames = [tuple(r.split("/")[1:3]) for r in sys.argv[3:]]
old, new = functions(sys.argv[1], renames), functions(sys.argv[2], [])
bad = 0
for k in sorted(set(old) | set(new)):
    a, b = old.get(k), new.get(k)
    same = a == b
    bad += not same
    print("%-9s %7s %7s  %s" % ("same" if same else "DIFFERENT", "-" if a is None else len(a), "-" if b is None else len(b), k))
print("%d functions, %d differ" % (len(set(old) | set(new)), bad))
sys.exit(1 if bad else 0)
