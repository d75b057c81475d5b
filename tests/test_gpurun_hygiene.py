"""Guards the tree the GPU box receives against lines the pool refuses outright (VERDICT r02:
round 2's driver GPU run was refused because one hipcc link line carried a bare sanitizer flag).

Scans every tracked source/script/build file that is NOT excluded by `.gpurunignore` (i.e. every
file that travels to the GPU box) for:
  * a hipcc/amdclang++ line with a sanitizer option that is neither directly after `-Xarch_host`
    nor accompanied by the gpu-sanitize opt-out (with no -Xarch_ option on that line);
  * XNACK-on builds or environments;
  * the scalar-cache store/writeback instruction names.
This file names those patterns itself, so it is listed in `.gpurunignore` (it is a CPU check)."""
import fnmatch
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SAN = "-f" + "sanitize="
OPT_OUT = "-fno-" + "gpu-sanitize"
XARCH = "-Xarch_"
SCANNED_EXT = (".sh", ".py", ".hip", ".cpp", ".h", ".c", ".jl", ".mk")
SCALAR_OPS = [p + q for p in ("s_" + "store", "s_" + "dcache_wb", "s_" + "dcache_inv", "s_" + "atomic",
                               "s_" + "buffer_store", "s_" + "scratch_store") for q in ("",)]


def _ignore_patterns():
    pats = []
    with open(os.path.join(ROOT, ".gpurunignore")) as f:
        for line in f:
            line = line.strip()
            if line and not line.startswith("#"):
                pats.append(line)
    return pats


def _ignored(rel, pats):
    for p in pats:
        if p.startswith("./"):
            pp = p[2:]
            # anchored at the top; a directory pattern covers everything beneath it
            if fnmatch.fnmatch(rel, pp) or rel.startswith(pp.rstrip("/") + "/"):
                return True
        else:
            parts = rel.split("/")
            for i in range(len(parts)):
                sub = "/".join(parts[i:])
                if fnmatch.fnmatch(sub, p) or fnmatch.fnmatch(parts[i], p):
                    return True
    return False


def _tree_files():
    """Every file beneath ROOT (relative paths), for a checkout without git metadata (an exported tree)."""
    files = []
    for base, dirs, names in os.walk(ROOT):
        dirs[:] = [d for d in dirs if d not in (".git", "__pycache__", ".pytest_cache")]
        files += [os.path.relpath(os.path.join(base, f), ROOT) for f in names]
    return files


def _travelling_files():
    try:
        out = subprocess.run(["git", "ls-files"], cwd=ROOT, capture_output=True, text=True, check=True).stdout
        untracked = subprocess.run(["git", "ls-files", "--others", "--exclude-standard"], cwd=ROOT,
                                   capture_output=True, text=True, check=True).stdout
        files = sorted(set(out.split()) | set(untracked.split()))
    except (OSError, subprocess.CalledProcessError):  # no git, or not a work tree: scan what is on disk
        files = sorted(_tree_files())
    pats = _ignore_patterns()
    return [f for f in files if (f.endswith(SCANNED_EXT) or os.path.basename(f) == "Makefile")
            and not _ignored(f, pats) and os.path.exists(os.path.join(ROOT, f))]


def _logical_lines(text):
    """Joins backslash continuations so one hipcc statement is one line."""
    return re.sub(r"\\\n", " ", text).split("\n")


def _bad_sanitizer_line(line):
    if SAN not in line:
        return False
    toks = line.split()
    for i, t in enumerate(toks):
        if SAN in t:
            prev = toks[i - 1] if i > 0 else ""
            if prev == XARCH + "host":
                continue
            if OPT_OUT in toks and not any(x.startswith(XARCH) for x in toks):
                continue
            return True
    return False


def test_ignore_matcher():
    pats = ["./tools/asan_host.sh", "*.log", "./gpurun_out"]
    assert _ignored("tools/asan_host.sh", pats)
    assert not _ignored("x/tools/asan_host.sh", pats)
    assert _ignored("a/b/c.log", pats)
    assert _ignored("gpurun_out/x/y.txt", pats)


def test_sanitizer_line_classifier():
    assert _bad_sanitizer_line("hipcc --offload-arch=gfx950 " + SAN + "address x.o")
    assert not _bad_sanitizer_line("hipcc " + XARCH + "host " + SAN + "address -c x.hip")
    assert not _bad_sanitizer_line("hipcc " + OPT_OUT + " " + SAN + "address x.o")
    assert _bad_sanitizer_line("hipcc " + OPT_OUT + " " + XARCH + "host -O1 " + SAN + "address x.o")


def test_no_refused_lines_in_files_that_travel_to_the_gpu_box():
    bad = []
    for rel in _travelling_files():
        with open(os.path.join(ROOT, rel), errors="replace") as f:
            text = f.read()
        for ln, line in enumerate(_logical_lines(text), 1):
            if _bad_sanitizer_line(line):
                bad.append(f"{rel}: bare sanitizer option: {line.strip()[:120]}")
            if "xnack+" in line or re.search(r"HSA_XNACK\s*=\s*1", line):
                bad.append(f"{rel}: xnack-on: {line.strip()[:120]}")
            for op in SCALAR_OPS:
                if re.search(r"\b" + op + r"\w*", line):
                    bad.append(f"{rel}: scalar-cache write instruction {op}: {line.strip()[:120]}")
    assert not bad, "\n".join(bad)


def test_sanitizer_build_files_are_gpurun_ignored():
    pats = _ignore_patterns()
    for rel in ("tools/asan_host.sh", "tests/test_asan_host.py", "tests/native/asan_driver.cpp",
                "tests/test_gpurun_hygiene.py"):
        assert _ignored(rel, pats), rel
