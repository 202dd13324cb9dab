"""A test-only stand-in for the part of NVIDIA Warp's Python API that the reference's Warp calculator is written against.

WHAT THIS MODELS.  It evaluates in float64 (Python floats).  It models WHAT THE SOURCE COMPUTES - the operations, their
order, the branches - not Warp's fp32 rounding, its code generation or its runtime.  It is written from Warp's public
definitions of the builtins below and holds no text of the reference; tests/golden/make_golden_warp.py is its one user.

  types      vec3, quat (xyzw), array (1-d, dtype vec3 / quat / float)
  decorators func, kernel (identity)
  builtins   tid, dot, length, cross, cw_mul, asin, sin, quat_rotate
  runtime    zeros, from_torch, to_torch, array.assign, launch, capture_begin / capture_end / capture_launch
             (a capture records the launches issued inside it; capture_launch replays them)

`quat_rotate` has two selectable definitions (`set_quat_rotate`):
  "matrix"  R(q) v with R the matrix of q AS GIVEN (no normalisation), built by oracle.hydro_oracle.rotation_from_quat_xyzw
            - the operation order that the Numba-executed fixtures pin, exact ties included;
  "warp"    Warp's own definition, v (2 w^2 - 1) + 2 w (u x v) + 2 u (u . v) with q = (u, w), which equals
            R(q) v + 2 (|q|^2 - 1) v: the same for a unit quaternion, different for any other.

Two things that Warp's generated code does and plain Python does not (`load_kernel_module`): every local of a function
is DECLARED ZERO-INITIALISED with the type of what is assigned to it, so
  * a local that is read on a path on which it was never assigned reads as a typed zero, and
  * a function that falls off its end returns zeros of the arity and types of its `return` statement.
`load_kernel_module` applies that rule to a source file through an `ast` pass and appends to `EVENTS` whenever either
case actually happens during a run.
"""
from __future__ import annotations

import ast
import math
import os
import sys
import types

import numpy as np

_REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _REPO not in sys.path:
    sys.path.insert(0, _REPO)
from oracle import hydro_oracle as _ho  # noqa: E402

IS_WARP_STANDIN = True
EVENTS: list = []                 # (kind, function, name) per zero-initialisation that mattered: "unassigned_local" / "fell_off_end"
_INF, _NAN = float("inf"), float("nan")


def _div(a: float, b: float) -> float:
    """IEEE division (Python raises on a zero divisor)."""
    try:
        return a / b
    except ZeroDivisionError:
        if a == 0.0 or a != a:
            return _NAN
        return math.copysign(_INF, a) * math.copysign(1.0, b)


# ------------------------------------------------------------------------------------------------------------ types
class vec3:
    __slots__ = ("x", "y", "z")
    _length = 3

    def __init__(self, x=0.0, y=None, z=None):
        if y is None:                                    # vec3(s): every component s
            y = z = x
        self.x, self.y, self.z = float(x), float(y), float(z)

    def __getitem__(self, i):
        return (self.x, self.y, self.z)[i]

    def __iter__(self):
        return iter((self.x, self.y, self.z))

    def __add__(self, o):
        return vec3(self.x + o.x, self.y + o.y, self.z + o.z)

    def __sub__(self, o):
        return vec3(self.x - o.x, self.y - o.y, self.z - o.z)

    def __neg__(self):
        return vec3(-self.x, -self.y, -self.z)

    def __mul__(self, s):
        if isinstance(s, vec3):
            raise TypeError("vec3 * vec3 is not defined; use cw_mul")
        s = float(s)
        return vec3(self.x * s, self.y * s, self.z * s)

    def __rmul__(self, s):
        s = float(s)
        return vec3(s * self.x, s * self.y, s * self.z)

    def __truediv__(self, s):
        s = float(s)
        return vec3(_div(self.x, s), _div(self.y, s), _div(self.z, s))

    def __repr__(self):
        return f"vec3({self.x!r}, {self.y!r}, {self.z!r})"


class quat:
    """x, y, z, w: the vector part first, as Warp stores it."""
    __slots__ = ("x", "y", "z", "w", "_matrix")
    _length = 4

    def __init__(self, x=0.0, y=0.0, z=0.0, w=0.0):
        self.x, self.y, self.z, self.w = float(x), float(y), float(z), float(w)
        self._matrix = None

    def __iter__(self):
        return iter((self.x, self.y, self.z, self.w))

    def __repr__(self):
        return f"quat({self.x!r}, {self.y!r}, {self.z!r}, {self.w!r})"


class array:
    """1-d array of `dtype` elements.  `array(dtype=...)` with no data is what a kernel signature's annotation builds."""

    def __init__(self, data=None, dtype=float, device=None, shape=None):
        self.dtype, self.device = dtype, device
        width = getattr(dtype, "_length", 0)
        if data is None:
            n = 0 if shape is None else int(shape)
            self._a = np.zeros((n, width) if width else (n,), dtype=np.float64)
        else:
            self._a = np.array(data, dtype=np.float64).reshape((-1, width) if width else (-1,))

    @property
    def shape(self):
        return (self._a.shape[0],)

    def __getitem__(self, i):
        row = self._a[i]
        if self.dtype is float:
            return float(row)
        return self.dtype(*row.tolist())

    def __setitem__(self, i, value):
        if self.dtype is float:
            self._a[i] = float(value)
            return
        if not isinstance(value, self.dtype):
            raise TypeError(f"array of {self.dtype.__name__}: cannot store {type(value).__name__}")
        self._a[i] = tuple(value)

    def assign(self, src):
        src = src._a if isinstance(src, array) else np.asarray(src, dtype=np.float64)
        if src.shape != self._a.shape:
            raise ValueError(f"assign: shape {src.shape} into {self._a.shape}")
        self._a[...] = src


def zeros(shape, dtype=float, device=None):
    return array(dtype=dtype, device=device, shape=shape)


def from_torch(t, dtype=float):
    """A tensor of shape (n, 3) / (n, 4) as n vec3 / quat (Warp wraps the memory; here the values are copied)."""
    return array(t.detach().cpu().numpy(), dtype=dtype)


def to_torch(a):
    import torch
    return torch.from_numpy(a._a.copy())


# --------------------------------------------------------------------------------------------------------- builtins
def func(f):
    return f


def kernel(f):
    return f


_tid = 0


def tid():
    return _tid


def dot(a, b):
    return a.x * b.x + a.y * b.y + a.z * b.z


def length(a):
    return math.sqrt(dot(a, a))


def cross(a, b):
    return vec3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x)


def cw_mul(a, b):
    return vec3(a.x * b.x, a.y * b.y, a.z * b.z)


def asin(x):
    try:
        return math.asin(x)
    except ValueError:
        return _NAN


def sin(x):
    try:
        return math.sin(x)
    except ValueError:
        return _NAN


QUAT_ROTATE_MODES = ("matrix", "warp")
_quat_rotate_mode = "matrix"


def set_quat_rotate(mode: str) -> None:
    global _quat_rotate_mode
    if mode not in QUAT_ROTATE_MODES:
        raise ValueError(f"quat_rotate: one of {QUAT_ROTATE_MODES}")
    _quat_rotate_mode = mode


def quat_rotate(q, v):
    if _quat_rotate_mode == "matrix":
        r = q._matrix
        if r is None:
            r = q._matrix = _ho.rotation_from_quat_xyzw((q.x, q.y, q.z, q.w)).tolist()
        return vec3(r[0][0] * v.x + r[0][1] * v.y + r[0][2] * v.z,
                    r[1][0] * v.x + r[1][1] * v.y + r[1][2] * v.z,
                    r[2][0] * v.x + r[2][1] * v.y + r[2][2] * v.z)
    u = vec3(q.x, q.y, q.z)
    return v * (2.0 * q.w * q.w - 1.0) + cross(u, v) * (2.0 * q.w) + u * (2.0 * dot(u, v))


# ---------------------------------------------------------------------------------------------------------- runtime
class _Graph:
    def __init__(self):
        self.launches = []


_capturing = None


def launch(kernel, dim, inputs=(), outputs=(), device=None):
    if _capturing is not None:                         # inside a capture nothing runs: the launch is recorded
        _capturing.launches.append((kernel, int(dim), tuple(inputs), tuple(outputs)))
        return
    global _tid
    for i in range(int(dim)):
        _tid = i
        kernel(*inputs, *outputs)
    _tid = 0


def capture_begin(device=None):
    global _capturing
    if _capturing is not None:
        raise RuntimeError("capture_begin inside a capture")
    _capturing = _Graph()


def capture_end(device=None):
    global _capturing
    graph, _capturing = _capturing, None
    if graph is None:
        raise RuntimeError("capture_end without capture_begin")
    return graph


def capture_launch(graph):
    for k, dim, ins, outs in graph.launches:
        launch(k, dim, ins, outs)


# ----------------------------------------------------------------------------- zero-initialised locals (the ast pass)
_UNSET = object()
_ZEROS = {"float": lambda: 0.0, "int": lambda: 0, "vec3": lambda: vec3(0.0), "quat": lambda: quat()}
_BUILTIN_TYPES = {"vec3": "vec3", "quat": "quat", "cross": "vec3", "quat_rotate": "vec3", "cw_mul": "vec3",
                  "dot": "float", "length": "float", "asin": "float", "sin": "float", "tid": "int"}


def _read_local(value, function, name, kind):
    if value is not _UNSET:
        return value
    EVENTS.append(("unassigned_local", function, name))
    return _ZEROS[kind]()


def _fell_off_end(function, kinds):
    EVENTS.append(("fell_off_end", function, None))
    out = tuple(_ZEROS[k]() for k in kinds)
    return out if len(out) > 1 else out[0]


class _FunctionPass:
    """One function: which local reads can happen before an assignment, whether its end is reachable, and the types
    needed to write the zeros.  Structured code only (if / for / while / return); anything else is refused."""

    def __init__(self, fn: ast.FunctionDef, alias: str, returns: dict):
        self.fn, self.alias, self.returns = fn, alias, returns
        self.types = {a.arg: self._annotation(a.annotation) for a in fn.args.args}
        self.params = set(self.types)
        self.early = []                                   # Name nodes (Load) that may be read unassigned
        self.return_types = None
        self.end_reachable = self._block(fn.body, set(self.params)) is not None

    # -- types ------------------------------------------------------------------------------------------------------
    def _is_api(self, node, names=None):
        return (isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id == self.alias
                and (names is None or node.attr in names))

    def _annotation(self, node):
        if node is None:
            return None
        if isinstance(node, ast.Name) and node.id in ("float", "int"):
            return node.id
        if self._is_api(node, ("vec3", "quat")):
            return node.attr
        if isinstance(node, ast.Call) and self._is_api(node.func, ("array",)):
            for kw in node.keywords:
                if kw.arg == "dtype":
                    return "array:" + str(self._annotation(kw.value))
        return None

    def _type(self, node):
        if isinstance(node, ast.Constant) and isinstance(node.value, (int, float)):
            return "float" if isinstance(node.value, float) else "int"
        if isinstance(node, ast.Name):
            return self.types.get(node.id)
        if isinstance(node, ast.UnaryOp):
            return self._type(node.operand)
        if isinstance(node, ast.BinOp):
            kinds = (self._type(node.left), self._type(node.right))
            if None in kinds:
                return None
            return "vec3" if "vec3" in kinds else ("float" if "float" in kinds or isinstance(node.op, ast.Div) else "int")
        if isinstance(node, ast.Subscript):
            base = self._type(node.value)
            if base and base.startswith("array:"):
                return base[6:]
            return "float" if base in ("vec3", "quat") else None
        if isinstance(node, ast.Tuple):
            return tuple(self._type(e) for e in node.elts)
        if isinstance(node, ast.Call):
            if isinstance(node.func, ast.Name):
                return node.func.id if node.func.id in ("float", "int") else self.returns.get(node.func.id)
            if self._is_api(node.func):
                return _BUILTIN_TYPES.get(node.func.attr)
        return None

    def _bind(self, target, kind):
        if isinstance(target, ast.Name):
            if kind is not None:
                self.types.setdefault(target.id, kind)
            return {target.id}
        if isinstance(target, ast.Tuple):
            kinds = kind if isinstance(kind, tuple) and len(kind) == len(target.elts) else (None,) * len(target.elts)
            return set().union(*(self._bind(t, k) for t, k in zip(target.elts, kinds)))
        return set()                                      # a store through a subscript binds no local

    # -- flow -------------------------------------------------------------------------------------------------------
    def _reads(self, node, assigned):
        for n in ast.walk(node):
            if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Load) and n.id in self.locals and n.id not in assigned:
                self.early.append(n)

    def _block(self, stmts, assigned):
        """Names certainly assigned after `stmts`, or None when every path through them has returned."""
        for s in stmts:
            if assigned is None:
                break                                     # unreachable
            if isinstance(s, ast.Expr):
                self._reads(s.value, assigned)
            elif isinstance(s, (ast.Assign, ast.AugAssign, ast.AnnAssign)):
                targets = s.targets if isinstance(s, ast.Assign) else [s.target]
                if s.value is not None:
                    self._reads(s.value, assigned)
                for t in targets:
                    if isinstance(s, ast.AugAssign) or not isinstance(t, (ast.Name, ast.Tuple)):
                        self._reads_of_target(t, assigned)
                    assigned = assigned | self._bind(t, self._type(s.value) if s.value is not None else None)
            elif isinstance(s, ast.If):
                self._reads(s.test, assigned)
                a, b = self._block(s.body, set(assigned)), self._block(s.orelse, set(assigned))
                assigned = b if a is None else a if b is None else a & b
            elif isinstance(s, (ast.For, ast.While)):
                if s.orelse:
                    raise NotImplementedError("loop with an else clause")
                self._reads(s.iter if isinstance(s, ast.For) else s.test, assigned)
                inner = set(assigned) | (self._bind(s.target, "int") if isinstance(s, ast.For) else set())
                self._block(s.body, inner)                # zero iterations are possible: nothing more is certain after
            elif isinstance(s, ast.Return):
                if s.value is not None:
                    self._reads(s.value, assigned)
                    kinds = self._type(s.value)
                    self.return_types = self.return_types or (kinds if isinstance(kinds, tuple) else (kinds,))
                assigned = None
            elif isinstance(s, ast.Pass):
                pass
            else:
                raise NotImplementedError(f"{type(s).__name__} in a kernel function")
        return assigned

    def _reads_of_target(self, target, assigned):
        """`x += e` and `a[i] = e` read x / a / i."""
        for n in ast.walk(target):
            if isinstance(n, ast.Name) and n.id in self.locals and n.id not in assigned:
                self.early.append(n)

    @property
    def locals(self):
        if not hasattr(self, "_locals"):
            self._locals = {n.id for n in ast.walk(self.fn) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Store)} - self.params
        return self._locals

    # -- rewrite ----------------------------------------------------------------------------------------------------
    def rewrite(self):
        fn, name = self.fn, self.fn.name
        early = {id(n): n for n in self.early}
        for n in early.values():
            if self.types.get(n.id) not in _ZEROS:
                raise NotImplementedError(f"{name}: cannot type the zero of local {n.id!r}")

        class Loads(ast.NodeTransformer):
            def visit_Name(inner, node):
                if id(node) not in early:
                    return node
                if not isinstance(node.ctx, ast.Load):
                    raise NotImplementedError(f"{name}: {node.id!r} is updated in place before it is assigned")
                return ast.copy_location(ast.Call(
                    func=ast.Name("__wp_read_local__", ast.Load()),
                    args=[node, ast.Constant(name), ast.Constant(node.id), ast.Constant(self.types[node.id])], keywords=[]), node)
        Loads().visit(fn)
        declare = [ast.Assign([ast.Name(v, ast.Store())], ast.Name("__wp_unset__", ast.Load()))
                   for v in sorted({n.id for n in early.values()})]
        tail = []
        if self.end_reachable and self.return_types is not None:
            if any(k not in _ZEROS for k in self.return_types):
                raise NotImplementedError(f"{name}: cannot type the zeros of its return value")
            tail = [ast.Return(ast.Call(func=ast.Name("__wp_fell_off_end__", ast.Load()),
                                        args=[ast.Constant(name), ast.Tuple([ast.Constant(k) for k in self.return_types], ast.Load())],
                                        keywords=[]))]
        doc = 1 if (fn.body and isinstance(fn.body[0], ast.Expr) and isinstance(getattr(fn.body[0], "value", None), ast.Constant)
                    and isinstance(fn.body[0].value.value, str)) else 0
        fn.body = fn.body[:doc] + declare + fn.body[doc:] + tail
        return bool(declare), bool(tail)


def load_kernel_module(path: str, name: str, alias: str = "wp"):
    """Execute the Warp source file `path` as module `name` with Warp's zero-initialisation rule applied, register it in
    `sys.modules` and return it.  `module.__wp_rewritten__` lists, per function, whether a local read and a fall-off-the-end
    return were rewritten.  Nothing is written next to `path`."""
    with open(path, "r", encoding="utf-8") as fh:
        tree = ast.parse(fh.read(), filename=path)
    returns, rewritten = {}, {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef):
            fp = _FunctionPass(node, alias, returns)
            if fp.return_types is not None:
                returns[node.name] = fp.return_types if len(fp.return_types) > 1 else fp.return_types[0]
            rewritten[node.name] = fp.rewrite()
    ast.fix_missing_locations(tree)
    mod = types.ModuleType(name)
    mod.__file__ = path
    mod.__dict__.update(__wp_read_local__=_read_local, __wp_fell_off_end__=_fell_off_end, __wp_unset__=_UNSET,
                        __wp_rewritten__=rewritten)
    sys.modules[name] = mod
    exec(compile(tree, path, "exec"), mod.__dict__)
    return mod


def install():
    """Make `import warp` find this module."""
    sys.modules["warp"] = sys.modules[__name__]
    return sys.modules[__name__]
