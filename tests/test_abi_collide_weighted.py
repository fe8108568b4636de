"""CPU-side checks of xpic_collide_weighted's boundary: the library exports it, the header's prototype and the package's
typed prototype agree, SYMBOLS lists it, and Context.collide_weighted returns the six keys (on a stand-in library: there
is no GPU here and no CPU fallback by design)."""
import ctypes as C
import os
import re
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CTYPES = {"xpic_ctx*": C.c_void_p, "int": C.c_int, "int64_t": C.c_int64, "double*": C.POINTER(C.c_double)}


def _header_prototype():
    txt = open(os.path.join(ROOT, "include", "xpic_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\b(\w+)\s+xpic_collide_weighted\s*\(([^)]*)\)\s*;", txt)
    assert m, "include/xpic_hip.h does not declare xpic_collide_weighted"
    args = []
    for a in m.group(2).split(","):
        a = " ".join(a.split())
        if a.endswith("]"):  # double out6[6]: a pointer
            a = re.sub(r"\s*\w+\[\d*\]$", "*", a)
        else:
            a = re.sub(r"\s*\b\w+$", "", a)  # (drop the parameter's name)
        args.append(a.replace(" *", "*"))
    return m.group(1), args


def test_header_package_and_export_agree():
    import xpic_amd as X

    ret, args = _header_prototype()
    assert ret == "int"
    assert args == ["xpic_ctx*", "int", "int", "const xpic_collision_params*", "int64_t", "double*"]
    want = [C.POINTER(X.CollisionParams) if a == "const xpic_collision_params*" else CTYPES[a] for a in args]
    assert "xpic_collide_weighted" in X.SYMBOLS
    if not os.path.exists(X.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    L = X.load_library()
    assert L.xpic_collide_weighted.restype is C.c_int
    assert list(L.xpic_collide_weighted.argtypes) == want
    assert hasattr(C.CDLL(X.LIB_PATH), "xpic_collide_weighted")
    # the struct the prototype points to: three 8-byte fields in the header's order
    assert [f[0] for f in X.CollisionParams._fields_] == ["strength", "dt", "seed"] and C.sizeof(X.CollisionParams) == 24


def test_collide_weighted_returns_the_six_keys():
    import xpic_amd as X

    seen = {}

    def fake(h, a, b, p, step, out):
        params = C.cast(p, C.POINTER(X.CollisionParams)).contents
        seen.update(h=h, a=a, b=b, step=step, strength=params.strength, dt=params.dt, seed=params.seed)
        for k, v in enumerate((7.0, 1.0, 0.25, 2.0, 5.0, 2.0)):
            out[k] = v
        return 0

    ctx = object.__new__(X.Context)
    ctx.L = types.SimpleNamespace(xpic_collide_weighted=fake)
    ctx.h = C.c_void_p(0)
    out = ctx.collide_weighted(0, 1, 2e-3, 11, seed=5, dt=0.7)
    assert out == dict(pairs=7, skipped=1, sigma2_sum=0.25, sigma2_over_1=2, heavy_updates=5, heavy_rejected=2)
    assert list(out) == ["pairs", "skipped", "sigma2_sum", "sigma2_over_1", "heavy_updates", "heavy_rejected"]
    assert all(isinstance(out[k], int) for k in out if k != "sigma2_sum") and isinstance(out["sigma2_sum"], float)
    assert (seen["a"], seen["b"], seen["step"], seen["strength"], seen["dt"], seen["seed"]) == (0, 1, 11, 2e-3, 0.7, 5)
    assert ctx.collide_weighted(1, 0, 1e-3, 0)["pairs"] == 7 and seen["dt"] == 0.0  # (dt None: the context's)
    ctx.h = None  # (nothing to destroy)
