"""The launch record of the 1-D decimated transforms (csrc/wx_dwt1d_trace.h, csrc/wx_debug.h, wx.dwt1d_trace()) without a device:
the three places that name the routes agree, the field count agrees, and the protocol refuses what the other records refuse."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "waveletsext.jl_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _enum_routes():
    """{id: name} of the WX_R1_* enum of wx_dwt1d_trace.h (first = 1, the others count on)"""
    body = re.search(r"enum\s*\{(.*?)\};", _read("wx_dwt1d_trace.h"), re.S).group(1)
    out, nxt = {}, 0
    for item in body.split(","):
        item = item.strip()
        if not item:
            continue
        m = re.fullmatch(r"WX_R1_(\w+)(?:\s*=\s*(\d+))?", item)
        assert m, item
        if m.group(2):
            nxt = int(m.group(2))
        out[nxt] = m.group(1)
        nxt += 1
    return out


def _comment_routes():
    """{id: name} of the table in the comment of wx_debug.h above WX_DWT1D_TRACE_FIELDS"""
    s = _read("wx_debug.h")
    block = s[s.index("Launch record of the 1-D decimated transforms"):s.index("#define WX_DWT1D_TRACE_FIELDS")]
    return {int(i): name for i, name in re.findall(r"^ \*\s+(\d+)  ([A-Z][A-Z0-9]+)\s", block, re.M)}


def test_routes_agree_between_header_comment_and_python(wx):
    enum = _enum_routes()
    assert enum == wx.DWT1D_ROUTES
    assert _comment_routes() == wx.DWT1D_ROUTES
    assert sorted(enum) == list(range(1, len(enum) + 1))


def test_field_count_agrees(wx):
    fields = int(re.search(r"#define WX_DWT1D_TRACE_FIELDS (\d+)", _read("wx_debug.h")).group(1))
    assert fields == len(wx.Dwt1dLaunch._fields)
    row = re.search(r"A row is WX_DWT1D_TRACE_FIELDS int32:\n \*\s+(.*)\n", _read("wx_debug.h")).group(1)
    assert len(row.split(",")) == fields
    cap = re.search(r"#define WX_DWT1D_TRACE_MAX \(1 << (\d+)\)", _read("wx_debug.h")).group(1)
    from waveletsext_jl_amd import _lib
    assert _lib.DWT1D_TRACE_MAX == 1 << int(cap)


def test_end_without_begin_is_an_argument_error(wx):
    lib = ctypes.CDLL(wx.LIB_PATH)
    row = (ctypes.c_int32 * 16)()
    assert lib.wx_debug_dwt1d_trace_end(row, ctypes.c_int(1)) == -2              # WX_EARG
    lib.wx_debug_dwt1d_trace_begin()
    assert lib.wx_debug_dwt1d_trace_end(row, ctypes.c_int(1)) == 0
    assert lib.wx_debug_dwt1d_trace_end(row, ctypes.c_int(1)) == -2


def test_every_hook_names_a_route_of_the_enum():
    """a WX_DWT1D_TRACE(...) in the dispatch code starts with a route of the enum (or the Float64 / Float32 choice between two)"""
    names = set(_enum_routes().values())
    seen = set()
    for f in ("wx_api.hip", "wx_dwt1d.hip"):
        for m in re.finditer(r"WX_DWT1D_TRACE\(([^,]+),", _read(f)):
            used = set(re.findall(r"WX_R1_(\w+)", m.group(1)))
            assert used and used <= names, (f, m.group(0))
            seen |= used
    assert seen == names, names - seen
