"""The README's "Environment knobs" table lists exactly the DVIE_* variables the code reads.

Read = named in a getenv("...") call under csrc/ or in os.environ.get("...") / os.environ["..."]
under the package.  Names that occur only inside `#ifdef DVIE_TIMING_DBG` regions (the timing
builds' ablation switches) are not part of the surface."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep_video_interpolation_extrapolation_amd")


def _csrc_names():
    """(names read outside timing regions, names read inside them)"""
    plain, timing = set(), set()
    csrc = os.path.join(PKG, "csrc")
    for fn in sorted(os.listdir(csrc)):
        if not fn.endswith((".hip", ".h", ".cpp")):
            continue
        stack = []  # one entry per open #if: True while inside a DVIE_TIMING_DBG region's first arm
        with open(os.path.join(csrc, fn)) as f:
            for line in f:
                s = line.strip()
                if re.match(r"#\s*if", s):
                    stack.append(bool(re.match(r"#\s*ifdef\s+DVIE_TIMING_DBG\b", s)))
                elif re.match(r"#\s*(else|elif)", s) and stack:
                    stack[-1] = False
                elif re.match(r"#\s*endif", s) and stack:
                    stack.pop()
                for name in re.findall(r'getenv\(\s*"(DVIE_[A-Z0-9_]+)"', line):
                    (timing if any(stack) else plain).add(name)
    return plain, timing


def _python_names():
    names = set()
    for d, _, files in os.walk(PKG):
        for fn in files:
            if fn.endswith(".py"):
                with open(os.path.join(d, fn)) as f:
                    src = f.read()
                names |= set(re.findall(r'os\.environ(?:\.get\(|\[)\s*"(DVIE_[A-Z0-9_]+)"', src))
    return names


def _readme_names():
    with open(os.path.join(ROOT, "README.md")) as f:
        text = f.read()
    sec = text.split("## Environment knobs", 1)[1].split("\n## ", 1)[0]
    names = set()
    for line in sec.splitlines():
        if line.startswith("|"):
            names |= set(re.findall(r"`(DVIE_[A-Z0-9_]+)`", line.split("|")[1]))
    return names


def test_readme_table_lists_exactly_the_variables_read():
    plain, timing = _csrc_names()
    read = plain | _python_names()
    assert plain and timing, "the scan found no getenv calls: has csrc/ moved?"
    assert "DVIE_PRECISION" in read and "DVIE_CONV_STRIP" in read
    table = _readme_names()
    assert read - table == set(), f"read by the code, missing from the README table: {sorted(read - table)}"
    assert table - read == set(), f"in the README table, read by no code: {sorted(table - read)}"

