"""CPU guard of the h16 range contract (csrc/common.h): every conversion of a data value from fp32 to the library's 16-bit format
saturates at the format's largest finite magnitude.  The sources may convert bare only where the value is bounded by construction
or is a weight, and such a line says why with an `h16-raw:` comment.  The GPU side of the contract is tests/test_h16_range_gpu.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deep3d_aerial_amd", "csrc")

# bare fp32 -> 16-bit conversions (the saturating forms pack_h16x2_sat / cvt_h16x4_sat do not match)
BARE = re.compile(r"\bpack_h16x2\(|\bcvt_h16x4\(|\(_Float16\)|\b__float2half_rn\(")
SATURATED = re.compile(r"\bsat_f16\(")           # the clamp the saturating helpers are built from
MARKER = "h16-raw:"
# common.h defines the conversions: inside these helpers a bare conversion is the point
HELPERS = {"pack_h16x2", "pack_h16x2_sat", "cvt_h16x4", "cvt_h16x4_sat", "round_h16", "sat_f16"}
DEF = re.compile(r"^__device__\s+__forceinline__\s+[\w:]+\s+(\w+)\(")


def scan(sources):
    """sources: {file name: text}.  Returns the "file:line: text" of every bare conversion that neither saturates nor carries
    the marker."""
    hits = []
    for name in sorted(sources):
        helper = None
        for n, line in enumerate(sources[name].splitlines(), 1):
            m = DEF.match(line)
            if m:
                helper = m.group(1)
            elif line.startswith("}"):
                helper = None
            code = line.split("//", 1)[0]
            if not BARE.search(code):
                continue
            if name == "common.h" and helper in HELPERS:
                continue
            if SATURATED.search(code) or MARKER in line:
                continue
            hits.append("%s:%d: %s" % (name, n, line.strip()))
    return hits


def _library_sources():
    out = {}
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".h", ".cpp", ".cu")):
            with open(os.path.join(CSRC, f)) as fh:
                out[f] = fh.read()
    return out


def test_scan_finds_bare_conversions_and_accepts_the_saturating_and_marked_ones():
    src = {
        "a.hip": "\n".join([
            "__device__ unsigned pack(float a, float b) { return pack_h16x2(a, b); }",           # 1: bare
            "x = cvt_h16x4(a, b, c, d);",                                                        # 2: bare
            "y = cvt_h16x4(a, b, c, d);   // h16-raw: a weight fragment",                       # 3: marked
            "z = pack_h16x2_sat(a, b);",                                                         # 4: the helper
            "*p = __float2half_rn(sat_f16(v));",                                                 # 5: clamped first
            "const _Float16 hv = (_Float16)v;",                                                  # 6: bare
            "q = __float2half_rn(v);   // RNE (a comment that says sat_f16( does not count)",    # 7: bare
            "// pack_h16x2(a, b) in a comment is not code",                                      # 8: comment
        ]),
        "common.h": "\n".join([
            "__device__ __forceinline__ unsigned pack_h16x2_sat(float a, float b) {",
            "    return pack_h16x2(sat_f16(a), sat_f16(b));",
            "}",
            "__device__ __forceinline__ unsigned other(float a) {",
            "    return pack_h16x2(a, 0.0f);",                                                    # 5: not a helper
            "}",
        ]),
    }
    hits = scan(src)
    assert [h.split(": ", 1)[0] for h in hits] == ["a.hip:1", "a.hip:2", "a.hip:6", "a.hip:7", "common.h:5"], hits


def test_every_h16_data_conversion_in_the_library_saturates():
    src = _library_sources()
    assert "common.h" in src and "pack_h16x2_sat" in src["common.h"]
    hits = scan(src)
    assert hits == [], "bare fp32 -> 16-bit conversions (saturate with pack_h16x2_sat / cvt_h16x4_sat / sat_f16, or say why " \
                       "the value is bounded with an `h16-raw:` comment):\n" + "\n".join(hits)
    # the exceptions stay few and each one says why
    marked = [(f, l) for f, t in src.items() for l in t.splitlines() if MARKER in l and BARE.search(l.split("//", 1)[0])]
    assert 0 < len(marked) <= 6, marked
    assert all(len(l.split(MARKER, 1)[1].strip()) >= 8 for _, l in marked), marked
