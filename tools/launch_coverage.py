#!/usr/bin/env python
"""Launch sites of cdlnet-video_amd/csrc/*.hip against a launch-trace log.

    python tools/launch_coverage.py                    # list the launch sites found in the sources
    python tools/launch_coverage.py trace.log          # ... and which of them a CDL_TRACE_FILE log reached
    python tools/launch_coverage.py trace.log --manifest tests/launch_coverage.json   # check / refresh the manifest

A launch site is one `kernel<<<...>>>` in the sources.  Its id is `<file>:<kernel with its template text>` (plus
`#n` for the n-th launch of the same text in a file), so ids survive edits that move lines.  A trace record names the
line of the CDL_LAUNCH_CHECK that follows the launch; a site inside a `#define` is reached through the lines that
use the macro.  Where several sites share one check line the record's note must name the kernel
(CDL_TRACE_NOTE("k_wgrad_l<%d,%d,%d>", ...)): a record that names none of them is reported as ambiguous.
"""
import argparse
import glob
import json
import os
import re
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cdlnet-video_amd", "csrc")
LAUNCH = re.compile(r"\b(k_\w+)\s*(<[^;<>()]*>)?\s*<<<")
LITERAL = re.compile(r"^(true|false|-?\d+)$")


class Site:
    def __init__(self, file, line, kernel, targs):
        self.file, self.line, self.kernel, self.targs = file, line, kernel, targs
        self.text = kernel + ("<" + ",".join(targs) + ">" if targs else "")
        self.id = None
        self.checks = set()            # lines a record of this site can carry
        if targs:
            args = ",".join(re.escape(a) if LITERAL.match(a) else r"[^,<>]+" for a in targs)
            self.named = re.compile(re.escape(kernel) + "<" + args + ">")
        else:
            self.named = re.compile(re.escape(kernel) + r"(?![\w<])")


def _define_blocks(lines):
    """[(first, last, name)] of the #define blocks (1-based, inclusive), continuation lines included."""
    out, i = [], 0
    while i < len(lines):
        m = re.match(r"\s*#\s*define\s+(\w+)", lines[i])
        if m:
            j = i
            while lines[j].rstrip().endswith("\\") and j + 1 < len(lines):
                j += 1
            out.append((i + 1, j + 1, m.group(1)))
            i = j + 1
        else:
            i += 1
    return out


def scan_file(path):
    name = os.path.basename(path)
    lines = open(path).read().split("\n")
    blocks = _define_blocks(lines)
    in_def = {}
    for a, b, nm in blocks:
        for ln in range(a, b + 1):
            in_def[ln] = (a, b, nm)
    checks = [i + 1 for i, ln in enumerate(lines) if "CDL_LAUNCH_CHECK()" in ln and (i + 1) not in in_def]

    def next_check(ln):
        for c in checks:
            if c >= ln:
                return c
        return None

    sites, seen = [], defaultdict(int)
    for i, ln in enumerate(lines):
        code = ln.split("//")[0]
        for m in LAUNCH.finditer(code):
            targs = [a.strip() for a in m.group(2)[1:-1].split(",")] if m.group(2) else []
            s = Site(name, i + 1, m.group(1), targs)
            seen[s.text] += 1
            s.id = f"{name}:{s.text}" + (f"#{seen[s.text]}" if seen[s.text] > 1 else "")
            blk = in_def.get(i + 1)
            if blk is None:
                c = next_check(i + 1)
                if c:
                    s.checks.add(c)
            else:
                a, b, nm = blk
                own = any("CDL_LAUNCH_CHECK()" in lines[k - 1] for k in range(i + 1, b + 1))
                uses = [k + 1 for k, l2 in enumerate(lines)
                        if (k + 1) not in in_def and re.search(r"\b" + nm + r"\s*\(", l2.split("//")[0])]
                for u in uses:
                    c = u if own else next_check(u)
                    if c:
                        s.checks.add(c)
            sites.append(s)
    return sites


def scan_sources(csrc=CSRC):
    sites = []
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        sites += scan_file(path)
    return sites


def parse_log(text, tests=None):
    """Records of a log.  A line `# test <id>` (a test runner may write one before each test) names the test the
    following records belong to; `tests`, when given, receives {record: first such id}."""
    recs, current = [], None
    for ln in text.splitlines():
        if ln.startswith("# test "):
            current = ln[7:].strip()
            continue
        parts = ln.split("\t")
        if len(parts) != 3 or ":" not in parts[0]:
            continue
        f, _, n = parts[0].rpartition(":")
        recs.append((f, int(n), parts[1], parts[2]))
        if tests is not None and current:
            tests.setdefault(recs[-1], current)
    return recs


def index(sites):
    by_check = defaultdict(list)
    for s in sites:
        for c in s.checks:
            by_check[(s.file, c)].append(s)
    return by_check


def site_of(by_check, rec):
    """The id of the launch site a record (file, line, launcher, note) belongs to; None when it fits none or several."""
    f, line, _, note = rec
    cands = by_check.get((f, line), [])
    if len(cands) > 1:
        flat = note.replace(" ", "")
        cands = [s for s in cands if s.named.search(flat)]
    return cands[0].id if len(cands) == 1 else None


def match(sites, recs):
    """-> ({site id: set of (launcher, note)}, [ambiguous or unmatched records])"""
    by_check = index(sites)
    reached, odd = defaultdict(set), []
    for rec in recs:
        sid = site_of(by_check, rec)
        if sid is None:
            odd.append(rec)
        else:
            reached[sid].add((rec[2], rec[3]))
    return reached, odd


def template_values(func):
    m = re.search(r"\[(.*)\]\s*$", func)
    return m.group(1) if m else ""


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("log", nargs="?", help="a CDL_TRACE_FILE log")
    ap.add_argument("--manifest", help="tests/launch_coverage.json: report sites missing from it")
    ap.add_argument("--update", action="store_true",
                    help="add the missing sites to the manifest: the first test of the log that reached them, or an empty waiver to fill in")
    ap.add_argument("--instances", action="store_true", help="print the template instantiations each site was reached with")
    a = ap.parse_args()
    sites = scan_sources()
    print(f"{len(sites)} launch sites in {len({s.file for s in sites})} files")
    first_test = {}
    if not a.log:
        for s in sites:
            print(f"  {s.id:70s} line {s.line}  checks {sorted(s.checks)}")
    else:
        tests = {}
        recs = parse_log(open(a.log).read(), tests)
        reached, odd = match(sites, recs)
        by_check = index(sites)
        for rec in recs:
            if rec in tests and site_of(by_check, rec):
                first_test.setdefault(site_of(by_check, rec), tests[rec])
        missed = [s for s in sites if s.id not in reached]
        print(f"{len(sites) - len(missed)} reached, {len(missed)} never reached:")
        for s in missed:
            print(f"  UNREACHED {s.id}  (line {s.line})")
        if a.instances:
            for s in sites:
                for inst in sorted({template_values(f) for f, _ in reached.get(s.id, ())}):
                    print(f"  {s.id}: [{inst}]")
        for r in odd:
            print("  UNMATCHED RECORD", r)
    if a.manifest:
        man = json.load(open(a.manifest)) if os.path.exists(a.manifest) else {}
        if a.update:
            for s in sites:
                if s.id not in man:
                    man[s.id] = {"test": first_test[s.id]} if s.id in first_test else {"waiver": ""}
            man = {s.id: man[s.id] for s in sites}
            with open(a.manifest, "w") as f:
                json.dump(man, f, indent=1)
                f.write("\n")
        missing = [s.id for s in sites if s.id not in man]
        stale = [k for k in man if k not in {s.id for s in sites}]
        for k in missing:
            print("  NOT IN MANIFEST", k)
        for k in stale:
            print("  STALE MANIFEST ENTRY", k)
        return 1 if missing or stale else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
