"""Record and replay the `clipperpy` calls a caller makes.  TEST INFRASTRUCTURE for tests/test_reference_files_on_shim.py.

`Recorder(shim).install()` registers a stand-in `clipperpy` (+ `.invariants`, `.utils`) whose classes and functions are the
shim's, wrapped: every construction, attribute assignment and method / function call is logged as a JSON-able event, with
the arrays it passed and the results it got back (arrays kept aside, referenced by key).  tests/golden/make_golden.py runs
the reference's unmodified plugin files through it once and stores the log as tests/golden/shim_trace_golden.npz.
`replay(segment, arrays, shim, objs)` issues the same calls, with the same arguments, on a shim again and returns every
result that differs from the recorded one: the reference's exact call sequence, kept as data, drives the shim where the
reference's sources are not present."""
import json
import types

import numpy as np

SHIM_MODULES = ("", "invariants", "utils")


def _shim_class(v):
    return isinstance(v, type) and getattr(v, "__module__", "").startswith("roman_amd.clipperpy")


class Recorder:
    def __init__(self, shim):
        self.shim = shim
        self.segments = []                          # [{"label": str, "events": [...]}]
        self.arrays = {}
        self.n_obj = 0

    # -- encoding
    def enc(self, v):
        if isinstance(v, _Obj):
            return {"ref": v._id}
        if isinstance(v, np.ndarray):
            k = f"a{len(self.arrays)}"
            self.arrays[k] = np.array(v, copy=True)
            return {"arr": k}
        if isinstance(v, np.bool_):
            return bool(v)
        if isinstance(v, np.integer):
            return int(v)
        if isinstance(v, np.floating):
            return float(v)
        if isinstance(v, (list, tuple)):
            return {"seq": [self.enc(x) for x in v], "tuple": isinstance(v, tuple)}
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        raise TypeError(f"cannot record a {type(v).__name__}")

    def log(self, ev):
        self.segments[-1]["events"].append(ev)

    def segment(self, label):
        self.segments.append({"label": label, "events": []})

    def ret(self, r):
        """-> (what the caller gets, its record): shim objects are wrapped and get an id, anything else is recorded as a value."""
        if _shim_class(type(r)):
            self.n_obj += 1
            return _Obj(self, r, self.n_obj), {"new": self.n_obj}
        return r, self.enc(r)

    # -- the stand-in module tree
    def install(self):
        import sys
        mods = {}
        for sub in SHIM_MODULES:
            real = self.shim if not sub else getattr(self.shim, sub)
            m = types.ModuleType("clipperpy" + ("." + sub if sub else ""))
            for name in dir(real):
                if name.startswith("_"):
                    continue
                v = getattr(real, name)
                path = (sub + "." if sub else "") + name
                if isinstance(v, types.ModuleType):
                    continue
                if isinstance(v, type):
                    setattr(m, name, _Cls(self, v, path))
                elif callable(v):
                    setattr(m, name, _Fn(self, v, path))
            mods[sub] = m
        for sub in SHIM_MODULES[1:]:
            setattr(mods[""], sub, mods[sub])
            sys.modules["clipperpy." + sub] = mods[sub]
        sys.modules["clipperpy"] = mods[""]
        return mods[""]

    def save(self, path, **extra):
        np.savez_compressed(path, trace=np.array(json.dumps(self.segments)), **{"arr_" + k: v for k, v in self.arrays.items()}, **extra)


def _unwrap(v):
    if isinstance(v, _Obj):
        return v._real
    if isinstance(v, (list, tuple)):
        return type(v)(_unwrap(x) for x in v)
    return v


def _call(rec, ev, f, a, kw):
    ev["args"] = [rec.enc(x) for x in a]
    ev["kw"] = {k: rec.enc(x) for k, x in kw.items()}
    rec.log(ev)
    r = f(*[_unwrap(x) for x in a], **{k: _unwrap(x) for k, x in kw.items()})
    out, ev["ret"] = rec.ret(r)
    return out


class _Cls:
    def __init__(self, rec, real, path):
        self._rec, self._real, self._path = rec, real, path

    def __call__(self, *a, **kw):
        self._rec.n_obj += 1
        oid = self._rec.n_obj
        ev = {"op": "new", "cls": self._path, "id": oid, "args": [self._rec.enc(x) for x in a], "kw": {k: self._rec.enc(x) for k, x in kw.items()}}
        self._rec.log(ev)
        return _Obj(self._rec, self._real(*[_unwrap(x) for x in a], **{k: _unwrap(x) for k, x in kw.items()}), oid)

    def __getattr__(self, name):                    # class constants (ROMAN.GEOMETRIC_MEAN, ...)
        return getattr(self._real, name)


class _Fn:
    def __init__(self, rec, real, path):
        self._rec, self._real, self._path = rec, real, path

    def __call__(self, *a, **kw):
        return _call(self._rec, {"op": "fn", "path": self._path}, self._real, a, kw)


class _Obj:
    def __init__(self, rec, real, oid):
        object.__setattr__(self, "_rec", rec)
        object.__setattr__(self, "_real", real)
        object.__setattr__(self, "_id", oid)

    def __getattr__(self, name):
        v = getattr(self._real, name)
        if callable(v) and not isinstance(v, type):
            return lambda *a, **kw: _call(self._rec, {"op": "call", "obj": self._id, "name": name}, v, a, kw)
        return v

    def __setattr__(self, name, value):
        self._rec.log({"op": "set", "obj": self._id, "name": name, "value": self._rec.enc(value)})
        setattr(self._real, name, _unwrap(value))


# ---- replay

def load(path):
    z = np.load(path, allow_pickle=False)
    arrays = {k[4:]: z[k] for k in z.files if k.startswith("arr_")}
    return json.loads(str(z["trace"])), arrays, z


def _resolve(shim, path):
    obj = shim
    for part in path.split("."):
        obj = getattr(obj, part)
    return obj


def _same(got, want):
    if isinstance(want, np.ndarray) or isinstance(got, np.ndarray):
        got, want = np.asarray(got), np.asarray(want)
        return got.shape == want.shape and np.array_equal(got, want, equal_nan=got.dtype.kind == "f")
    if isinstance(want, (list, tuple)):
        return isinstance(got, (list, tuple)) and len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))
    return got == want


def replay(segment, arrays, shim, objs):
    """Issue the events of one recorded segment on `shim` (objects live in `objs` across segments) -> list of
    (event, what the shim returned now) where that differs from what it returned when the trace was recorded."""
    def dec(v):
        if isinstance(v, dict):
            if "ref" in v:
                return objs[v["ref"]]
            if "arr" in v:
                return arrays[v["arr"]].copy()
            if "seq" in v:
                s = [dec(x) for x in v["seq"]]
                return tuple(s) if v["tuple"] else s
        return v

    bad = []
    for ev in segment["events"]:
        args = [dec(x) for x in ev.get("args", [])]
        kw = {k: dec(x) for k, x in ev.get("kw", {}).items()}
        if ev["op"] == "new":
            objs[ev["id"]] = _resolve(shim, ev["cls"])(*args, **kw)
            continue
        if ev["op"] == "set":
            setattr(objs[ev["obj"]], ev["name"], dec(ev["value"]))
            continue
        f = getattr(objs[ev["obj"]], ev["name"]) if ev["op"] == "call" else _resolve(shim, ev["path"])
        r = f(*args, **kw)
        want = ev["ret"]
        if isinstance(want, dict) and "new" in want:
            objs[want["new"]] = r
        elif not _same(r, dec(want)):
            bad.append((ev, r))
    return bad
