#!/usr/bin/env python3
"""Compare the kernels' instruction sequences between two hipcc -S --cuda-device-only listings (tools/kernel_resources.py says
how to make one): per kernel of the named namespaces "identical" — the same instructions in the same order, label names apart —
or both instruction counts.
   python3 tools/kernel_bodies.py parent.s branch.s smafa_join smafa_cc chimera ..."""
import re, subprocess, sys


def bodies(path):
    """{demangled kernel name: [instruction, ...]} with comments dropped and labels numbered in order of appearance"""
    out, name, lines = {}, None, []
    for line in open(path):
        m = re.match(r"(_Z\w+):\s", line)
        if m and name is None:
            name, lines = m.group(1), []
        elif name and line.startswith(".Lfunc_end"):
            out[name], name = lines, None
        elif name:
            text = line.split(";")[0].strip()
            if text and (not text.startswith(".") or text.startswith(".LBB")):
                lines.append(text)
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True).stdout.split("\n")
    res = {}
    for dem, body in zip(names, out.values()):
        labels = {}
        for tok in re.findall(r"\.LBB\d+_\d+", "\n".join(body)):
            labels.setdefault(tok, "L%d" % len(labels))
        res[dem.split("(")[0].replace("void ", "")] = [re.sub(r"\.LBB\d+_\d+", lambda t: labels[t.group(0)], b) for b in body]
    return res


def count(body):
    return sum(1 for b in body if not b.endswith(":"))


old, new = bodies(sys.argv[1]), bodies(sys.argv[2])
for name in sorted(new):
    if name.split("::")[0] not in sys.argv[3:] or name not in old:
        continue
    same = old[name] == new[name]
    print("%-40s %s" % (name, "identical" if same else "differs: %d instructions, were %d" % (count(new[name]), count(old[name]))))
