#!/usr/bin/env python3
"""Mutation check of tests/test_rule_actors_exact.py (CPU, the emulated kernels): copies of the tree with one defect planted in
magent_amd/csrc/actors.hip or actors_dev.h each must FAIL the new file; the same copies are put through tests/test_rule_actors.py
to see what the suite noticed before.  Prints one block per defect (tests/README.md keeps the result).

    python tools/mutation_actors.py [a b c d e]
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFECTS = {   # name -> (what, file, text, replacement)
    "a": ("kth_cell without `before +=`", "actors.hip", "        before += cnt;\n", ""),
    "b": ("slot 1 replaced by slot 0", "actors.hip",
          "draw(a.seed, a.counter, (uint32_t)i, 1, (uint32_t)a.attack_base)", "draw(a.seed, a.counter, (uint32_t)i, 0, (uint32_t)a.attack_base)"),
    "c": ("(uint32_t)h for h >> 32", "actors_dev.h", "return (uint32_t)(h >> 32) % m;", "return (uint32_t)h % m;"),
    "d": ("mypos from __ffsll instead of the highest lane", "actors.hip",
          "if (m_me) mypos = base + 63 - __clzll(m_me);", "if (m_me) mypos = base + __ffsll(m_me) - 1;"),
    "e": ("counter truncated to 32 bits in draw", "actors_dev.h", "mix64(counter + 0x9E3779B97F4A7C15ull)", "mix64((uint32_t)counter + 0x9E3779B97F4A7C15ull)"),
}


def pytest_on(tree, files):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    p = subprocess.run([sys.executable, "-m", "pytest", "-m", "not gpu", "-q", "-p", "no:cacheprovider", "--tb=line"] + files,
                       cwd=tree, env=env, capture_output=True, text=True)
    failed = re.findall(r"^FAILED (\S+)", p.stdout, re.M)
    lines = [l for l in p.stdout.splitlines() if re.match(r"^E  .*(Error|assert)", l)]
    return p.returncode, failed, lines, p.stdout.strip().splitlines()[-1:]


def main(names):
    for name in names:
        what, fname, text, replacement = DEFECTS[name]
        with tempfile.TemporaryDirectory(prefix="actors_mut_") as tmp:
            tree = os.path.join(tmp, "tree")
            shutil.copytree(ROOT, tree, symlinks=True, ignore=shutil.ignore_patterns(".git", "_build","__pycache__", "*.o"))
            path = os.path.join(tree, "magent_amd", "csrc", fname)
            src = open(path).read()
            assert src.count(text) == 1, "defect (%s) does not apply to %s" % (name, fname)
            open(path, "w").write(src.replace(text, replacement))
            print("== (%s) %s" % (name, what))
            for files in (["tests/test_rule_actors_exact.py"], ["tests/test_rule_actors.py"]):
                rc, failed, lines, tail = pytest_on(tree, files)
                print("  %s: exit code %d, %s" % (files[0], rc, tail[0] if tail else ""))
                for f in failed:
                    print("    FAILED " + f)
                for l in lines[:3]:
                    print("    " + l[:300])
            sys.stdout.flush()


if __name__ == "__main__":
    main(sys.argv[1:] or sorted(DEFECTS))
