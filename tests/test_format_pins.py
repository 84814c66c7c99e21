"""CPU test: the printf FORMAT STRINGS of the reference's row writers must occur verbatim in the front end, each in the
file under popscle_amd/host/ that holds its writer (.best: cmd_demuxlet.hpp; the files of freemuxlet: table_writers.hpp).

The writers themselves (hprintf over htsFile) need htslib and cannot be compiled here, so rows
a10 / b10 of SURVEY section 8 stay unpinned as code; what CAN be pinned is the text that decides every printed column:
the header lines and the conversion specifications of .best (cmd_cram_demuxlet.cpp:629,993), .lmix
(cmd_cram_freemux2.cpp:112,161), .clust1.samples.gz (:661,663) and the .clust1.vcf.gz header and record pieces (:609-656).
The strings were extracted from those lines of the reference's source files into tests/golden/format_pins.json
(`python tests/test_format_pins.py <reference checkout>` writes it again), so the test needs nothing outside the
repository."""
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "popscle_amd", "host")
GOLDEN = os.path.join(ROOT, "tests", "golden", "format_pins.json")

CASES = [
    ("cmd_cram_demuxlet.cpp", [629, 993]),                      # .best header and row
    ("cmd_cram_freemux2.cpp", [112, 161]),                      # .lmix header and row
    ("cmd_cram_freemux2.cpp", [661, 663]),                      # .clust1.samples.gz header and row
    ("cmd_cram_freemux2.cpp", list(range(609, 657))),           # .clust1.vcf.gz header lines and record pieces
]
# the file of the front end that holds the writer of each case
HOLDER = ["cmd_demuxlet.hpp", "table_writers.hpp", "table_writers.hpp", "table_writers.hpp"]

_LIT = re.compile(r'"((?:[^"\\]|\\.)*)"')


def literals_of(text):
    """C string literals of a source text, adjacent ones (separated by white space only) concatenated; comments
    stripped first"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out, pos = [], 0
    cur, end = None, None
    for m in _LIT.finditer(text):
        line_start = text.rfind("\n", 0, m.start()) + 1
        if "//" in _LIT.sub('""', text[line_start:m.start()]):
            continue  # inside a // comment
        if cur is not None and text[end:m.start()].strip() == "":
            cur += m.group(1)
        else:
            if cur is not None:
                out.append(cur)
            cur = m.group(1)
        end = m.end()
    if cur is not None:
        out.append(cur)
    return out


def ref_formats(ref_dir, fname, lines):
    src = open(os.path.join(ref_dir, fname)).read().split("\n")
    got = []
    for ln in lines:
        got += [s for s in literals_of(src[ln - 1]) if "\\t" in s or "%" in s or s.startswith("##")]
    return got


def golden_formats(fname, lines):
    for rec in json.load(open(GOLDEN)):
        if rec["file"] == fname and rec["lines"] == lines:
            return rec["formats"]
    raise KeyError((fname, lines))


def product_text(holder):
    return "\x00".join(literals_of(open(os.path.join(HOST, holder)).read()))


@pytest.mark.parametrize("fname,lines", CASES)
def test_reference_format_strings_occur_in_the_front_end(fname, lines):
    holder = HOLDER[CASES.index((fname, lines))]
    want = golden_formats(fname, lines)
    assert len(want) >= min(len(lines), 14), (fname, lines, want)
    have = product_text(holder)
    for s in want:
        # the reference writes %lf / %lg; printf treats the l as a no-op for doubles, the front end keeps it as written
        assert s in have, f"{fname}: format string of lines {lines} not found in {holder}: {s!r}"


if __name__ == "__main__":
    recs = [{"file": f, "lines": ls, "formats": ref_formats(sys.argv[1], f, ls)} for f, ls in CASES]
    with open(GOLDEN, "w") as fh:
        json.dump(recs, fh, indent=1)
        fh.write("\n")
