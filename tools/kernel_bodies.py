#!/usr/bin/env python3
"""Compare the kernels' instruction sequences between two hipcc -S --cuda-device-only listings (tools/kernel_resources.py says
how to make one): per kernel "identical" — the same instructions in the same order, label names apart — or both instruction
counts.  With namespace arguments only the kernels of those namespaces, without any every kernel of the listings; -q prints only
the kernels that are not identical.  Exits 1, naming the kernels (mangled too), if a body differs or a kernel is in one listing
only; the last line is "N kernels, M identical".
   python3 tools/kernel_bodies.py [-q] parent.s branch.s [smafa_join smafa_cc chimera ...]"""
import re, subprocess, sys


def bodies(path):
    """{mangled kernel name: [instruction, ...]} with comments dropped and labels numbered in order of appearance"""
    raw, name, lines = {}, None, []
    for line in open(path):
        m = re.match(r"(_Z\w+):\s", line)
        if m and name is None:
            name, lines = m.group(1), []
        elif name and line.startswith(".Lfunc_end"):
            raw[name], name = lines, None
        elif name:
            text = line.split(";")[0].strip()
            if text and (not text.startswith(".") or text.startswith(".LBB")):
                lines.append(text)
    out = {}
    for name, body in raw.items():
        labels = {}
        for tok in re.findall(r"\.LBB\d+_\d+", "\n".join(body)):
            labels.setdefault(tok, "L%d" % len(labels))
        out[name] = [re.sub(r"\.LBB\d+_\d+", lambda t: labels[t.group(0)], b) for b in body]
    return out


def count(body):
    return sum(1 for b in body if not b.endswith(":"))


args = [a for a in sys.argv[1:] if a != "-q"]
quiet = len(args) < len(sys.argv) - 1
old, new = bodies(args[0]), bodies(args[1])
mangled = sorted(set(old) | set(new))
shown = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True).stdout.split("\n")
shown = {m: d.split("(")[0].replace("void ", "") for m, d in zip(mangled, shown)}  # (a kernel's arguments say nothing its name does not)
wanted = [m for m in mangled if not args[2:] or shown[m].split("::")[0] in args[2:]]
bad = []
for m in sorted(wanted, key=lambda m: (shown[m], m)):
    if m not in old or m not in new:
        verdict = "only in %s" % (args[1] if m in new else args[0])
    elif old[m] == new[m]:
        verdict = "identical"
    else:
        verdict = "differs: %d instructions, were %d" % (count(new[m]), count(old[m]))
    if verdict != "identical":
        bad.append(m)
        print("%-40s %s  [%s]" % (shown[m], verdict, m))
    elif not quiet:
        print("%-40s %s" % (shown[m], verdict))
for m in bad:
    print("NOT IDENTICAL: %s  [%s]" % (shown[m], m), file=sys.stderr)
print("%d kernels, %d identical" % (len(wanted), len(wanted) - len(bad)))
sys.exit(1 if bad else 0)
