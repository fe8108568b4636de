"""include/xpic_hip.h as tests/test_abi.py reads it: the one parser of its prototypes, structs, macros and enums."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    """the header's text without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xpic_hip.h")).read(), flags=re.S)


def symbols():
    return sorted(set(re.findall(r"\b(xpic_[a-zA-Z0-9_]+)\s*\(", header())))


def prototypes():
    """{name: (return type, argument types)} of every function the header declares, the parameter names dropped; an array
    parameter (`double out6[6]`) is a pointer, `(void)` no argument"""
    out = {}
    for ret, name, args in re.findall(r"^\s*([\w ]+?\*?)\s*\b(xpic_\w+)\s*\(([^)]*)\)\s*;", header(), flags=re.M):
        types = []
        for a in args.split(","):
            a = " ".join(a.split())
            if a == "void":
                continue
            a = re.sub(r"\s*\w+\[\d*\]$", "*", a) if a.endswith("]") else re.sub(r"\s*\b\w+$", "", a)
            types.append(a.replace(" *", "*"))
        out[name] = (ret.strip(), types)
    return out


def structs():
    """the names of the structs the header defines (the opaque xpic_ctx has no body)"""
    return re.findall(r"typedef struct (\w+) \{", header())


def struct_fields(name):
    """the members of a struct as "type name", one per member (`double q, m, n` declares three)"""
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header(), flags=re.S)
    assert m, name
    out = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if "(*" in decl:  # a function pointer: one member, as it is written
            out.append(decl)
        elif decl:
            typ, rest = decl.split(" ", 1)
            out += ["%s %s" % (typ, v.strip()) for v in rest.split(",")]
    return out


def member_names(name):
    """the members' names, in the header's order"""
    return [re.search(r"\(\*(\w+)\)", f).group(1) if "(*" in f else f.split()[-1].split("[")[0] for f in struct_fields(name)]


def macro(name):
    """the integer value of `#define name value` (plain, hexadecimal or in parentheses)"""
    return int(re.search(r"#define %s \(?(-?\w+)\)?" % name, header()).group(1), 0)


def enum(name):
    """{enumerator: value} of `enum name`"""
    body = re.search(r"enum %s \{(.*?)\};" % name, header(), flags=re.S).group(1)
    return {k: int(v) for k, v in re.findall(r"(\w+) = (\d+)", body)}
