"""Per-kernel comparison of two sets of device ISA listings (`hipcc <flags of the object> --cuda-device-only -S`):
    tools/isa_diff.py old.s new.s
    tools/isa_diff.py old.s [old2.s ...] -- new.s [new2.s ...]     (a translation unit that was split or merged)
    tools/isa_diff.py --demangle ...     (functions and kernel metadata are keyed by the demangled name with
                                          `(anonymous namespace)::` removed, not by the mangled one: a type or a function that
                                          moved between a named and an anonymous namespace, which changes every mangled name
                                          it appears in; needs c++filt)
Prints SAME / DIFF, the instruction counts and the (mangled) name of every function of either side.  Comments and assembler
directives are dropped and local labels normalised (.LBB<n>_<m>: <n> is the function's index in the file and shifts when a
function is added or removed), so a refactor of host code or of other kernels must come out as SAME for a kernel it did not touch.
A function is DIFF as well when it is missing on one side, defined more than once on one side (DUP), or when its kernel
metadata differ (registers, LDS, scratch, spills: META, with the two values).  The last line counts each verdict; the exit
status is 1 unless everything is SAME."""
import hashlib
import re
import subprocess
import sys

META = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count",
        "sgpr_spill_count")


def bodies(path, out, dup):
    cur, funcs = None, set()
    for line in open(path):
        t = re.match(r"^\s+\.type\s+(_Z\w+),@function", line)
        if t:
            funcs.add(t.group(1))
        m = re.match(r"^(_Z\w+):", line)
        if m and m.group(1) in funcs:   # (a data object -- an LDS array of a library template -- has a label too)
            cur = m.group(1)
            if cur in out:
                dup.add(cur)
            out[cur] = []
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            ins = re.sub(r"\.L(BB|tmp|func_\w+?)\d+_", ".L_", line.split(";")[0].strip())
            if ins and not ins.startswith("."):
                out[cur].append(ins)


def metadata(path, out):
    """{kernel name: {field: value}} from the amdhsa.kernels list of the listing's metadata note"""
    entry = {}
    for line in open(path):
        m = re.match(r"^  (- | {2})\.(\w+):\s*(\S*)", line)
        if not m:
            continue
        if m.group(1) == "- ":
            entry = {}
        if m.group(2) == "name":
            out[m.group(3)] = entry
        elif m.group(2) in META:
            entry[m.group(2)] = int(m.group(3))


def side(paths):
    body, dup, meta = {}, set(), {}
    for p in paths:
        bodies(p, body, dup)
        metadata(p, meta)
    return body, dup, meta


def digest(body):
    return hashlib.sha1("\n".join(body).encode()).hexdigest() if body is not None else None


def demangled(names):
    """{mangled: demangled name without `(anonymous namespace)::`} through c++filt, one name per line.  DF16_ (_Float16) is
    handed over as Dh (half), so a _Float16 parameter prints as `half`: a c++filt that does not know DF16_ yet leaves the
    whole name mangled."""
    names = sorted(names)
    out = subprocess.run(["c++filt"], input="\n".join(n.replace("DF16_", "Dh") for n in names) + "\n", capture_output=True,
                         text=True, check=True).stdout.splitlines()
    assert len(out) == len(names), "c++filt answered %d lines for %d names" % (len(out), len(names))
    return {n: d.replace("(anonymous namespace)::", "") for n, d in zip(names, out)}


def rekey(body, dup, meta):
    """the three tables of a side keyed by demangled(); two functions that now share a key are a DUP"""
    key = demangled(set(body) | set(meta))
    nbody, ndup = {}, {key[k] for k in dup}
    for k, v in body.items():
        if key[k] in nbody:
            ndup.add(key[k])
        nbody[key[k]] = v
    return nbody, ndup, {key[k]: v for k, v in meta.items()}


args = sys.argv[1:]
demangle = "--demangle" in args
if demangle:
    args.remove("--demangle")
if "--" in args:
    old, new = args[:args.index("--")], args[args.index("--") + 1:]
else:
    old, new = args[:1], args[1:]
a, adup, ameta = side(old)
b, bdup, bmeta = side(new)
if demangle:
    a, adup, ameta = rekey(a, adup, ameta)
    b, bdup, bmeta = rekey(b, bdup, bmeta)
count = {}
for k in sorted(set(a) | set(b)):
    verdict, note = "SAME", ""
    if k in adup or k in bdup:
        verdict, note = "DIFF", " DUP"
    elif digest(a.get(k)) != digest(b.get(k)):
        verdict = "DIFF"
    elif ameta.get(k) != bmeta.get(k):
        verdict, note = "DIFF", " META %s -> %s" % (ameta.get(k), bmeta.get(k))
    count[verdict] = count.get(verdict, 0) + 1
    print(verdict, len(a.get(k, [])), len(b.get(k, [])), k[:72] + note)
spills = sum(m.get("vgpr_spill_count", 0) + m.get("sgpr_spill_count", 0) for m in bmeta.values())
scratch = sorted(m["private_segment_fixed_size"] for m in bmeta.values() if m.get("private_segment_fixed_size"))
print("%d functions: %d SAME, %d DIFF; new side: %d kernels with metadata, %d spilled registers, scratch bytes %s"
      % (sum(count.values()), count.get("SAME", 0), count.get("DIFF", 0), len(bmeta), spills, scratch))
sys.exit(0 if count.get("DIFF", 0) == 0 else 1)
