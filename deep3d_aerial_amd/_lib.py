"""ctypes binding of the C-ABI library (include/deep3d_planesweep.h).

The library is built in-tree by deep3d_aerial_amd/csrc/Makefile (see __graft_entry__.build).
There is NO fallback: if the shared object is missing or lacks a symbol, importing the
operators raises, and every operator refuses tensors that are not on the GPU.
"""
import ctypes
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# D3D_LIBRARY: load another build of the library (tools/run_ab.sh links its -D variants to a scratch path and points this
# at them, so the in-tree production library is never overwritten by an experiment).  Read once, at import.
SO_PATH = os.environ.get("D3D_LIBRARY") or os.path.join(CSRC, "libdeep3d_planesweep.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "deep3d_planesweep.h")


class LibraryMissing(RuntimeError):
    pass


# the scalar types the header is written in; its typedefs (d3d_stream_t) join them as they are read
_CTYPES = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "long long": ctypes.c_longlong,
           "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}


def parse_header(text):
    """The ABI a C header states, as ctypes: ({function: (argtypes, restype)}, {struct: ctypes.Structure subclass},
    {D3D_* constant: int}).  A pure function of the text, for the subset of C that include/deep3d_planesweep.h is written in:
    `#define D3D_NAME <integer>`, typedefs of a known type, `typedef struct { ... } name;` and prototypes of d3d_ functions.
    Every pointer is a c_void_p, whatever it points to (the header cannot tell host from device memory); a `const char*`
    return is a c_char_p.  Whatever else it meets is a ValueError that names the function or struct and the text."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"#\s*ifdef\s+__cplusplus.*?#\s*endif", " ", text, flags=re.S)   # extern "C" { and its }
    types, protos, structs, consts = dict(_CTYPES), {}, {}, {}

    def ctype(spec, where):
        spec = " ".join(w for w in spec.replace("*", " * ").split() if w != "const")
        if "*" not in spec and spec not in types:
            raise ValueError("%s: unknown type %r" % (where, spec))
        return ctypes.c_void_p if "*" in spec else types[spec]

    def declarator(decl, where):
        """`const float* depth` | `R[9]` -> (type text, name, array length or None)."""
        m = re.fullmatch(r"\s*(.*?)\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*", decl, flags=re.S)
        if not m:
            raise ValueError("%s: cannot read %r" % (where, " ".join(decl.split())))
        return m.groups()

    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(D3D_\w+)(.*)$", text, flags=re.M):
        m = re.fullmatch(r"\s+\(?\s*(-?\d+)\s*\)?\s*", value)
        if not m:
            raise ValueError("#define %s: %r is not an integer" % (name, value.strip()))
        consts[name] = int(m.group(1))
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)

    def struct(m):
        body, name = m.groups()
        fields = []
        for line in filter(None, (d.strip() for d in body.split(";"))):
            decls = [declarator(d, name) for d in line.split(",")]
            spec = decls[0][0]
            if len(decls) > 1 and ("*" in spec or any(d[0] for d in decls[1:])):   # `float *a, *b`: the header has none
                raise ValueError("%s: cannot read %r" % (name, line))
            t = ctype(spec, "%s: %r" % (name, line))
            fields += [(field, t * int(n) if n else t) for _, field, n in decls]
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
        return " "

    text = re.sub(r"\btypedef\s+struct\s+\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        m = re.fullmatch(r"typedef (.+?) ?(\w+)", stmt)
        if m:
            types[m.group(2)] = ctype(m.group(1), "typedef " + m.group(2))
            continue
        m = re.fullmatch(r"(.+?) ?\b(d3d_\w+) ?\(([^()]*)\)", stmt)
        if not m:
            raise ValueError("cannot read the declaration %r" % stmt)
        ret, name, params = m.groups()
        args = []
        for param in ([] if params.strip() == "void" else params.split(",")):
            spec, _, n = declarator(param, name)
            if n:
                raise ValueError("%s: array parameter %r" % (name, param.strip()))
            args.append(ctype(spec, "%s(%s)" % (name, param.strip())))
        protos[name] = (args, ctypes.c_char_p if ret.replace(" ", "") == "constchar*" else ctype(ret, name))
    return protos, structs, consts


def header_text(path=HEADER):
    try:
        with open(path) as f:
            return f.read()
    except OSError as e:
        raise LibraryMissing("the header %s cannot be read: the binding is derived from it" % path) from e


# One statement of the ABI: the header's.  SIGNATURES is name -> argtypes, or (argtypes, restype) where the function does
# not return int; STRUCTS and CONSTANTS are what ortho / mesh / fuse / _runtime take their records and limits from.
PROTOTYPES, STRUCTS, CONSTANTS = parse_header(header_text())
SIGNATURES = {name: args if ret is ctypes.c_int else (args, ret) for name, (args, ret) in PROTOTYPES.items()}
ABI_VERSION = CONSTANTS["D3D_ABI_VERSION"]
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_HIP = (CONSTANTS["D3D_ERR_" + n] for n in ("INVALID_ARG", "UNSUPPORTED", "HIP"))


def build(verbose=False):
    """hipcc --offload-arch=gfx950 build of the C-ABI library, in-tree (cross-compiles on CPU)."""
    cmd = ["make", "-C", CSRC, "-j4", "libdeep3d_planesweep.so"]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise RuntimeError("building libdeep3d_planesweep.so failed")
    return SO_PATH


_lib = None


def load():
    """Load the library and bind every symbol the header declares. Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise LibraryMissing(
            "%s not found -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C deep3d_aerial_amd/csrc`. There is no CPU fallback." % SO_PATH)
    lib = ctypes.CDLL(SO_PATH)
    for name, sig in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise LibraryMissing("symbol %s missing from %s" % (name, SO_PATH)) from e
        fn.argtypes, fn.restype = sig if isinstance(sig, tuple) else (sig, ctypes.c_int)
    if lib.d3d_version() != ABI_VERSION:
        raise LibraryMissing("ABI version mismatch: library %d, binding %d" % (lib.d3d_version(), ABI_VERSION))
    _lib = lib
    return lib


def h16_format():
    """"f16" | "bf16": the 16-bit operand format the loaded library was built with (d3d_h16_format, ABI 9)."""
    return load().d3d_h16_format().decode("ascii")


def code_objects(path=None):
    """The gfx950 code objects (ELF images, as bytes) bundled in the built library's .hip_fatbin section."""
    import struct

    data = open(path or SO_PATH, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    pos = data.find(magic)
    while pos >= 0:
        n = struct.unpack_from("<Q", data, pos + 24)[0]
        q = pos + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, q)
            triple = data[q + 24:q + 24 + tl]
            q += 24 + tl
            if b"amdgcn" not in triple or size == 0:
                continue
            elf = data[pos + off:pos + off + size]
            if elf[:4] == b"\x7fELF":
                yield elf
        pos = data.find(magic, pos + len(magic))


def kernel_code_table(path=None):
    """{mangled name: (size, SHA-256)} of the gfx950 machine code of every kernel (function symbol) in `path`: the built
    library by default, or a single .o -- both carry the offload bundle.  Two builds produce the same machine code exactly
    if their tables are equal, which is how a refactor of a kernel is held to "nothing changed":
        a, b = kernel_code_table("parent/planesweep_tiled.o"), kernel_code_table("planesweep_tiled.o")
        assert a.keys() == b.keys() and not [n for n in a if a[n] != b[n]]
    A name that more than one code object defines is ambiguous and maps to None."""
    import hashlib
    import struct

    table = {}
    for elf in code_objects(path):
        shoff, = struct.unpack_from("<Q", elf, 0x28)
        shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
        secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
        for sh in secs:
            if sh[1] != 2:   # SHT_SYMTAB
                continue
            strtab = secs[sh[6]]
            for k in range(sh[5] // sh[9]):
                st_name, st_info, _, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", elf, sh[4] + k * sh[9])
                if (st_info & 0xF) != 2 or st_size == 0 or st_shndx >= len(secs):   # STT_FUNC
                    continue
                end = elf.index(b"\0", strtab[4] + st_name)
                name = elf[strtab[4] + st_name:end].decode("ascii", "replace")
                sec = secs[st_shndx]
                o = sec[4] + (st_value - sec[3])
                table[name] = None if name in table else (st_size, hashlib.sha256(elf[o:o + st_size]).hexdigest())
    return table


def kernel_code_sha256(symbol_prefix, path=None):
    """SHA-256 of the gfx950 machine code of ONE kernel in the built library: the bytes of the (unique) function symbol whose
    mangled name starts with `symbol_prefix`, read from the code objects bundled in the .so's .hip_fatbin section.  A counter
    profile of a kernel stays valid exactly as long as this hash does -- an edit elsewhere in the same source file does not
    invalidate it, a change of compiler flags does (bench.profiled_traffic, tools/profile_round.sh).  None if not found."""
    found = [entry for name, entry in kernel_code_table(path).items() if name.startswith(symbol_prefix)]
    return found[0][1] if len(found) == 1 and found[0] else None


def check(rc, what):
    if rc != 0:
        msg = load().d3d_last_error().decode("utf-8", "replace")
        kind = {ERR_INVALID_ARG: "invalid argument", ERR_UNSUPPORTED: "unsupported", ERR_HIP: "HIP error"}.get(rc, "error %d" % rc)
        raise RuntimeError("%s failed (%s): %s" % (what, kind, msg))
