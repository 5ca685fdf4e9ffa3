#!/usr/bin/env python3
"""Mutation check of tests/test_engine_buffers.py (CPU, the emulated kernels ONLY): copies of the tree with one defect planted in the engine's
output writers each must FAIL the new file; the same copies are put through the CPU legs of the suite that existed before
(tests/test_emu_parity.py) to see what it noticed.  Prints one block per defect (tests/README.md keeps the result).

These mutants write out of bounds on purpose.  On the emulator the guards belong to the same host allocation, so that is harmless; they are
never built into the product library and never run in a `gpu` leg: the copies are tested with -m "not gpu" and have no library of their own.

    python tools/mutation_buffers.py [a b c d e]
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFECTS = {   # name -> (what, file, text, replacement)
    "a": ("k_render_fast rounds the tail's float4 count up: up to 12 bytes past the end", "render.hip",
          "const int nq = remain >= (size_t)(64 * 7) ? 16 * 7 : (int)(remain >> 2);", "const int nq = remain >= (size_t)(64 * 7) ? 16 * 7 : (int)((remain + 3) >> 2);"),
    "b": ("k_render_fast's bf16-cell store without its k < total_cells guard", "render.hip",
          "if (k < total_cells) __builtin_nontemporal_store(o, (cell16_t *)R.view + k);", "__builtin_nontemporal_store(o, (cell16_t *)R.view + k);"),
    "c": ("k_get_reward without its row guard: a whole workgroup writes rows past n", "step.hip",
          "if (i < G.n) out[i] = G.next_reward[i] + group_reward;", "out[i] = G.next_reward[i < G.n ? i : 0] + group_reward;"),
    "d": ("render_block's bf16-cell form skips the cells outside the view range: a stale interior, no overrun", "kernels_dev.h",
          "if (valid[u]) __builtin_nontemporal_store(v, (cell16_t *)R.view + (k0 + lane));", "if (valid[u] && mask[cellv[u]]) __builtin_nontemporal_store(v, (cell16_t *)R.view + (k0 + lane));"),
    "e": ("the batched pipeline's folded get_reward writes every group's rows one row further", "pipe.hip",
          "it.counts, it.rewards[g], it.group_reward[g]);", "it.counts, it.rewards[g] ? it.rewards[g] + 1 : nullptr, it.group_reward[g]);"),
}


# the legs of the suite before this file that run the same writers on the emulator: every scenario against the oracle, the forced render
# kernels (float32 and bf16 cells), the batched pipeline with and without groups left out
OLD = ["tests/test_emu_parity.py", "-k", "match_oracle or battle_render_kernels or test_emulated_batched_pipeline"]


def pytest_on(tree, files):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    p = subprocess.run([sys.executable, "-m", "pytest", "-m", "not gpu", "-q", "-p", "no:cacheprovider", "--tb=line"] + files,
                       cwd=tree, env=env, capture_output=True, text=True)
    failed = re.findall(r"^FAILED (\S+)", p.stdout, re.M)
    lines = [l for l in p.stdout.splitlines() if re.search(r"AssertionError: ", l)]
    return p.returncode, failed, lines, p.stdout.strip().splitlines()[-1:]


def main(names):
    for name in names:
        what, fname, text, replacement = DEFECTS[name]
        with tempfile.TemporaryDirectory(prefix="buffers_mut_") as tmp:
            tree = os.path.join(tmp, "tree")
            shutil.copytree(ROOT, tree, symlinks=True, ignore=shutil.ignore_patterns(".git", "_build", "__pycache__", "*.o", "lib", "_ref"))
            path = os.path.join(tree, "magent_amd", "csrc", fname)
            src = open(path).read()
            assert src.count(text) == 1, "defect (%s) does not apply to %s" % (name, fname)
            open(path, "w").write(src.replace(text, replacement))
            print("== (%s) %s" % (name, what))
            for files in (["tests/test_engine_buffers.py"], OLD):
                rc, failed, lines, tail = pytest_on(tree, files)
                print("  %s: exit code %d, %s" % (files[0], rc, tail[0] if tail else ""))
                for f in failed[:12]:
                    print("    FAILED " + f)
                if len(failed) > 12:
                    print("    ... %d more" % (len(failed) - 12))
                for l in lines[:2]:
                    print("    " + l[:420])
            sys.stdout.flush()


if __name__ == "__main__":
    main(sys.argv[1:] or sorted(DEFECTS))
