"""Per-kernel comparison of two device ISA listings (`hipcc <flags of the object> --cuda-device-only -S`): tools/isa_diff.py old.s new.s
Prints SAME / DIFF, the instruction counts and the mangled name of every function of either file.  Comments and assembler
directives are dropped and local labels normalised (.LBB<n>_<m>: <n> is the function's index in the file and shifts when a
function is added or removed), so a refactor of host code or of other kernels must come out as SAME for a kernel it did not touch."""
import hashlib
import re
import sys


def bodies(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            ins = re.sub(r"\.L(BB|tmp|func_\w+?)\d+_", ".L_", line.split(";")[0].strip())
            if ins and not ins.startswith("."):
                out[cur].append(ins)
    return out


def digest(body):
    return hashlib.sha1("\n".join(body).encode()).hexdigest() if body is not None else None


a, b = bodies(sys.argv[1]), bodies(sys.argv[2])
for k in sorted(set(a) | set(b)):
    print("SAME" if digest(a.get(k)) == digest(b.get(k)) else "DIFF", len(a.get(k, [])), len(b.get(k, [])), k[:72])
