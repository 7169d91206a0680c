"""Dev tool: the launch sequence of hicom_amd/csrc/executor.hip on the CPU, for "same launches" reviews of executor changes.

Compiles an executor.hip (host side only, the project's flags), links it against stub.cpp -- which logs every kernel entry point,
event call and stop event instead of launching -- and runs stub.cpp's matrix of hicom_compressor_args once per setting of the
executor's environment switches (a process each: the switches are read once).  No GPU, about 3 s per compile.

    python tools/executor_trace/run.py                    # log of the working tree's executor.hip on stdout
    python tools/executor_trace/run.py --rev HEAD         # ... of a committed one
    python tools/executor_trace/run.py --diff HEAD~1      # unified diff of that revision's log against the working tree's (empty = same)
    python tools/executor_trace/run.py --rev HEAD --coverage    # + executor.hip lines with a launch call that no case reached
"""
from __future__ import annotations

import argparse
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
from hicom_amd.build_native import FLAGS, hipcc  # noqa: E402  (plain module: no torch, no build on import)

REL = "hicom_amd/csrc/executor.hip"
SETTINGS = [{}] + [{k: v} for k, v in (
    ("HICOM_TAIL_LAUNCHES", "3"), ("HICOM_TAIL_LAUNCHES", "4"), ("HICOM_TAIL_LAUNCHES", "5"), ("HICOM_CHAIN_WIDE", "0"), ("HICOM_CHAIN_WIDE", "1"),
    ("HICOM_RING_MARG", "1"), ("HICOM_FOLD_EVENTS", "0"), ("HICOM_SHARD_TAIL", "0"), ("HICOM_STREAM_FIRST", "0"), ("HICOM_ADAPT_PAIR", "0"),
    ("STUB_CAPTURING", "1"))] + [
    {"HICOM_TAIL_LAUNCHES": "3", "STUB_TAIL_EUNSUP": "1"}, {"HICOM_TAIL_LAUNCHES": "3", "HICOM_RING_MARG": "1"},
    {"HICOM_TAIL_LAUNCHES": "5", "HICOM_RING_MARG": "1"}, {"HICOM_TAIL_LAUNCHES": "5", "HICOM_CHAIN_WIDE": "1"},
    {"HICOM_FOLD_EVENTS": "0", "HICOM_SHARD_TAIL": "0"}, {"STUB_CAPTURING": "1", "HICOM_FOLD_EVENTS": "0"},
] + [{"STUB_FAIL_AT": str(n)} for n in range(1, 25)]       # the n-th launch / event call of every case fails: same stop, same code
SWITCHES = sorted({k for s in SETTINGS for k in s} | {"HICOM_GLOBAL_NARROW", "HICOM_GLOBAL_NO_MARG", "HICOM_RING_WPW"})


SITE = re.compile(r"\bCHK\(|\breturn hicom_\w+\(")      # a launch call site: `CHK(...)` or a bare `return hicom_...(...)`


def sites_of(text):
    return [n for n, l in enumerate(text, 1) if SITE.search(l) and not l.lstrip().startswith(("//", "#define"))]


def build(src: str, work: str, coverage: bool) -> str:
    cc = hipcc()
    csrc = os.path.join(work, "hicom_amd", "csrc")
    os.makedirs(csrc)
    os.makedirs(os.path.join(work, "include"))
    shutil.copy(os.path.join(ROOT, "include", "hicom_hip.h"), os.path.join(work, "include"))
    shutil.copy(os.path.join(ROOT, "hicom_amd", "csrc", "common.hpp"), csrc)
    text = open(src).read().splitlines()
    if coverage:      # hicom_trace_hit(<line>) in front of the call of every site, as `0 +` in front of its return code: no line moves
        for n in sites_of(text):
            text[n - 1] = re.sub(r"\bCHK\(", f"CHK(hicom_trace_hit({n}) + ", re.sub(r"\breturn (hicom_\w+\()", rf"return hicom_trace_hit({n}) + \1", text[n - 1]))
        text[0] = 'extern "C" int hicom_trace_hit(int); ' + text[0]
    with open(os.path.join(csrc, "executor.hip"), "w") as f:
        f.write("\n".join(text) + "\n")
    exe = os.path.join(work, "trace")
    # (executor.hip at the same relative path in every build, compiled from inside `work`: nothing in the object depends on where `src` lies)
    subprocess.check_call([cc, *FLAGS, "-c", REL, "-o", "executor.o"], cwd=work)
    subprocess.check_call([cc, "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-x", "c++", "-I", os.path.join(os.path.dirname(os.path.dirname(cc)), "include"),
                           "-c", os.path.join(HERE, "stub.cpp"), "-o", "stub.o"], cwd=work)
    subprocess.check_call([cc, "executor.o", "stub.o", "-o", exe], cwd=work)
    return exe


def trace(src: str, coverage: bool = False) -> str:
    with tempfile.TemporaryDirectory() as work:
        exe = build(src, work, coverage)
        hits = os.path.join(work, "hits")
        out = []
        for setting in SETTINGS:
            env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
            env.update(setting)
            if coverage:
                env["STUB_HITS"] = hits
            r = subprocess.run([exe], env=env, capture_output=True, text=True)
            out.append("==== " + (" ".join(f"{k}={v}" for k, v in setting.items()) or "(default)") + f" : exit {r.returncode}\n" + r.stdout + r.stderr)
        if coverage:
            text = open(src).read().splitlines()
            hit = {int(l) for l in open(hits)} if os.path.exists(hits) else set()
            missed = [n for n in sites_of(text) if n not in hit]
            out.append(f"==== coverage: {len(sites_of(text))} launch call sites, {len(sites_of(text)) - len(missed)} reached\n" +
                       "".join(f"    not reached: executor.hip:{n}: {text[n - 1].strip()[:110]}\n" for n in missed))
    return "".join(out)


def source_of(rev, work: str) -> str:
    if rev is None:
        return os.path.join(ROOT, REL)
    path = os.path.join(work, "executor_" + re.sub(r"\W", "_", rev) + ".hip")
    with open(path, "w") as f:
        f.write(subprocess.check_output(["git", "show", f"{rev}:{REL}"], cwd=ROOT, text=True))
    return path


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rev", help="git revision whose executor.hip is traced (default: the working tree)")
    ap.add_argument("--src", help="path of an executor.hip to trace instead")
    ap.add_argument("--diff", metavar="REV", help="diff REV's log against the working tree's")
    ap.add_argument("--coverage", action="store_true", help="append the launch call sites that no case reached (each site gets a hit counter in front of it)")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as work:
        if args.diff:
            old, new = trace(source_of(args.diff, work)), trace(source_of(None, work))
            sys.stdout.writelines(difflib.unified_diff(old.splitlines(True), new.splitlines(True), args.diff, "working tree"))
            print(f"{old.count(chr(10) + 'case ')} cases in {len(SETTINGS)} processes: " + ("logs identical" if old == new else "LOGS DIFFER"))
            return 0 if old == new else 1
        sys.stdout.write(trace(args.src or source_of(args.rev, work), args.coverage))
    return 0


if __name__ == "__main__":
    sys.exit(main())
