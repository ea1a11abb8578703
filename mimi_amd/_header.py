"""Reader for include/mimi_hip.h: the ctypes view of the C ABI, taken from the header's own text (standard library only:
no compiler, no library load).  Not a C parser: the header is written in a narrow subset -- integer #defines, enums with
explicit values, opaque handle typedefs, flat structs and prototypes over int / int32_t / int64_t / double /
unsigned char / size_t and pointers -- and exactly that subset is read.  Anything else raises ValueError with the
offending text; no declaration ever falls back to a default type."""
import ctypes as C
import keyword
import re
from types import SimpleNamespace

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double,
           "unsigned char": C.c_ubyte, "size_t": C.c_size_t}
_INTEGER = r"-?(?:0[xX][0-9a-fA-F]+|\d+)"
_DECLARATION = re.compile(r"(unsigned char|\w+)\s*(\**)\s*(\w*)\s*(?:\[(\d+)\])?")


def _declaration(text, known, named):
    """`[const] type [*] [name] [[n]]` -> (ctype, name, n or None): a scalar is exact, a handle and a pointer to a type the
    header knows are c_void_p; `named` says whether a name has to be there (fields, parameters) or must not (returns).
    known: type name -> its ctype by value, None where it exists behind a pointer only (void, char, the structs)."""
    m = _DECLARATION.fullmatch(re.sub(r"\bconst\b", " ", text).strip())
    if not m or bool(m.group(3)) != named:
        raise ValueError(f"not a declaration this reader knows: {text!r}")
    base, stars, name, count = m.groups()
    if stars and (len(stars) > 1 or base not in known):
        raise ValueError(f"pointer to an unknown type: {text!r}")
    if not stars and known.get(base) is None:
        raise ValueError(f"unknown scalar type: {text!r}")
    return C.c_void_p if stars else known[base], name, int(count) if count else None


def _fields(body, known):
    """the ordered (name, ctype) list of a struct body; `double a, b;` declares several, `lambda` becomes `lambda_`"""
    out = []
    for line in filter(None, (l.strip() for l in body.split(";"))):
        first, *more = [d.strip() for d in line.split(",")]
        if more and "*" in line:
            raise ValueError(f"several pointer declarators on one line: {line!r}")
        ctype, name, count = _declaration(first, known, named=True)
        of_type = first[:first.rindex(name)]
        for d, n in [(name, count)] + [_declaration(of_type + d, known, named=True)[1:] for d in more]:
            out.append((d + "_" if keyword.iskeyword(d) else d, ctype * n if n else ctype))
    return out


def _statements(text):
    """the top-level declarations, each up to its `;` outside braces; the `}` that closes extern "C" is skipped"""
    text, wrapped = re.subn(r'extern\s+"C"\s*\{', " ", text)
    depth, start = 0, 0
    for i, ch in enumerate(text):
        if ch == "{":
            depth += 1
        elif ch == "}":
            depth -= 1
            if depth < 0 and wrapped and not text[start:i].strip():
                depth, wrapped, start = 0, 0, i + 1
            elif depth < 0:
                raise ValueError(f"unbalanced braces: {text[start:i + 1].strip()!r}")
        elif ch == ";" and depth == 0:
            yield " ".join(text[start:i].split())
            start = i + 1
    if text[start:].strip():
        raise ValueError(f"unfinished declaration: {text[start:].strip()!r}")


def parse(text):
    """-> namespace with
         functions  name -> (restype, [argtypes])     ctypes types; restype None for void, c_char_p for const char*
         structs    name -> [(field, ctype)]          in the header's order
         enums      enumerator -> value               of every enum
         defines    name -> value                     `#define NAME <integer literal>` only"""
    h = SimpleNamespace(functions={}, structs={}, enums={}, defines={})
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    h.defines.update((m.group(1), int(m.group(2), 0))
                     for m in re.finditer(rf"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+({_INTEGER})[ \t]*$", text, flags=re.M))
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    known = {**SCALARS, "void": None, "char": None}
    for s in _statements(text):
        if m := re.fullmatch(r"enum \w+ \{(.*)\}", s):
            for e in m.group(1).split(","):
                if not (v := re.fullmatch(rf"\s*(\w+)\s*=\s*({_INTEGER})\s*", e)):
                    raise ValueError(f"enumerator without an explicit integer value: {e.strip()!r} in {s!r}")
                h.enums[v.group(1)] = int(v.group(2), 0)
        elif m := re.fullmatch(r"typedef struct \w+\s?\* ?(\w+_t)", s):
            known[m.group(1)] = C.c_void_p
        elif m := re.fullmatch(r"typedef struct (\w+) \{([^{}]*)\} ?(\w+)", s):
            if m.group(1) != m.group(3):
                raise ValueError(f"struct tag and typedef name differ: {s!r}")
            h.structs[m.group(1)] = _fields(m.group(2), known)
            known[m.group(1)] = None
        elif m := re.fullmatch(r"([\w\s*]+?)\s*\b(\w+) ?\(([^()]*)\)", s):
            ret, name, params = m.groups()
            if name in h.functions:
                raise ValueError(f"declared twice: {s!r}")
            restype = None if ret == "void" else _declaration(ret, known, named=False)[0]
            if re.fullmatch(r"const char ?\*", ret):
                restype = C.c_char_p
            h.functions[name] = (restype, [] if params.strip() == "void" else
                                 [C.c_void_p if count else ctype
                                  for ctype, _, count in (_declaration(p, known, named=True) for p in params.split(","))])
        else:
            raise ValueError(f"not a declaration this reader knows: {s!r}")
    return h
