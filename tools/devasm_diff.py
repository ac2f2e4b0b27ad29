"""Is the device code of two trees the same?   python tools/devasm_diff.py TREE_A TREE_B [file.hip ...]
Every source of radargnn_amd/build.py (or the named ones) -> gfx950 assembly with that build's flags (kept in TREE/tools/var/asm/),
minus the per-compile `__hip_cuid_` lines; prints per file "identical" or the first differing line and the kernel it is in."""
import glob, os, re, subprocess, sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from radargnn_amd.build import EXTRA_FLAGS, FLAGS, SOURCES, _hipcc


def asm(tree, name):
    out = os.path.join(tree, "tools", "var", "asm", name.replace(".hip", ".s"))
    deps = glob.glob(os.path.join(tree, "radargnn_amd", "csrc", "*")) + glob.glob(os.path.join(tree, "include", "*"))
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run([_hipcc(), *FLAGS, *EXTRA_FLAGS.get(name, []), "--cuda-device-only", "-S",
                        os.path.join(tree, "radargnn_amd", "csrc", name), "-o", out], check=True)
    return [l for l in open(out) if "__hip_cuid_" not in l]


a, b, names = sys.argv[1], sys.argv[2], sys.argv[3:] or SOURCES
with ThreadPoolExecutor(max_workers=8) as ex:
    got = list(ex.map(lambda j: asm(*j), [(t, n) for n in names for t in (a, b)]))
for i, name in enumerate(names):
    x, y = got[2 * i], got[2 * i + 1]
    d = next((k for k in range(min(len(x), len(y))) if x[k] != y[k]), None if len(x) == len(y) else min(len(x), len(y)))
    if d is None:
        print(f"{name}: identical ({len(x)} lines)")
    else:
        kern = next((m.group(1) for l in reversed(x[:d + 1]) if (m := re.match(r"^(\w+):", l))), "?")
        print(f"{name}: DIFFERS at line {d + 1}, in or after `{kern}`\n  A: {x[d].rstrip() if d < len(x) else '<end>'}\n  B: {y[d].rstrip() if d < len(y) else '<end>'}")
