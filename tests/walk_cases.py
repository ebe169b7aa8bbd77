"""Inputs of the record-walk shape tests (tests/test_gpu_walk_shapes.py): the decoder fuzz's slices
(staging_cases.py) wrapped into layouts whose field offsets depend on the data, a dense string case for
the walk's register path, and a seeded generator of random walk layouts.

Every layout is held here as a small tree (Node) from which both the copybook text and the record bytes
come: the record generator states the layout a second time, independently of the oracle's walk -- an
OCCURS DEPENDING ON array takes its count from the dependee value emitted earlier in the record, a null
dependee keeps the previous entry, an out-of-range count means the maximum, a string dependee goes
through its occurs_mappings.  The generator returns each record's true length as it emitted it, which
tests/test_walk_cases.py compares with the oracle's VarOccursRecordExtractor framing.
tests/test_walk_cases.py pins this module on the CPU: a generator bug would silently drop coverage.
"""
from __future__ import annotations

import functools
import random
import re
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

import staging_cases as S
from cobrix_amd.codepages import lut_for, utf8_lut
from test_decode_fuzz import _random_ascii_bytes, _random_bytes

N_REC = 321          # five tiles of 64 records and one record
WHOLE_SHARE = 0.7    # records emitted whole; the others are cut at a uniform length
WRAPPERS = ("behind", "inside", "fixed")


@dataclass
class Node:
    """A statement of a layout: a primitive (pic, size, gen) or a group (children)."""
    name: str
    pic: str = ""                                   # the clause after the name ("PIC 9(1)", "COMP-2")
    size: int = 0
    gen: Optional[Callable] = None                  # rng (numpy Generator) -> the field's bytes
    children: Optional[List["Node"]] = None
    occurs: Optional[Tuple[Optional[int], int]] = None   # (min, max); min None: a fixed OCCURS max
    dep: Optional[str] = None                       # DEPENDING ON name
    handlers: Dict[str, int] = field(default_factory=dict)   # occurs_mappings of the array
    redefines: Optional[str] = None
    count: Optional[str] = None                     # a dependee: "zoned" / "comp" / "comp3" / "str"
    count_max: int = 0                              # the largest in-range count of the arrays using it
    seg: Optional[str] = None                       # a segment redefine: the segment id it is active for


def copybook_text(body: List[Node], record: str = "R") -> str:
    out = [f"       01  {record}."]

    def line(n: Node, depth: int):
        pad = " " * (7 + 2 * depth)
        parts = [f"{pad}{5 * depth:02d}  {n.name}"]
        if n.redefines:
            parts.append(f"REDEFINES {n.redefines}")
        if n.pic:
            parts.append(n.pic)
        if n.occurs:
            lo, hi = n.occurs
            parts.append(f"OCCURS {hi} TIMES" if lo is None else f"OCCURS {lo} TO {hi} TIMES DEPENDING ON {n.dep}")
        text = " ".join(parts) + "."
        if len(text) > 72:      # columns past 72 are comments: the OCCURS clause on a line of its own
            text = " ".join(parts[:-1]) + "\n" + pad + "      " + parts[-1] + "."
        assert max(map(len, text.split("\n"))) <= 72, text
        out.append(text)
        for c in n.children or []:
            line(c, depth + 1)

    for n in body:
        line(n, 1)
    return "\n".join(out) + "\n"


def occurs_mappings(body: List[Node]) -> Dict[str, Dict[str, int]]:
    out: Dict[str, Dict[str, int]] = {}

    def visit(n: Node):
        if n.handlers:
            out[n.name] = dict(n.handlers)
        for c in n.children or []:
            visit(c)

    for n in body:
        visit(n)
    return out


def leaf_names(body: List[Node]) -> List[str]:
    out: List[str] = []

    def visit(n: Node):
        if n.children is None:
            if n.name != "FILLER":
                out.append(n.name.replace("-", "_"))   # as the parser transforms identifiers
        else:
            for c in n.children:
                visit(c)

    for n in body:
        visit(n)
    return out


# ------------------------------------------------------------------------------------------------
# count fields: (bytes, registered value) -- value None: the field decodes to null and the dependee map
# keeps its previous entry
# ------------------------------------------------------------------------------------------------
def _ebcdic_or_ascii(s: str, ascii: bool) -> bytes:
    return s.encode("ascii" if ascii else "cp037")


def draw_count(rng, n: Node, ascii: bool = False):
    """A dependee's bytes: in-range, out-of-range and non-numeric values."""
    hi = n.count_max
    u = rng.random()
    if n.count == "str":     # PIC X(2): Right(trimmed string); the arrays map A / B / C
        s = ["A ", "B ", "C ", "ZZ", "  "][int(rng.integers(0, 5))]
        return _ebcdic_or_ascii(s, ascii), s.strip()
    if u < 0.7:
        v = int(rng.integers(0, hi + 1))
    else:
        v = int(rng.integers(hi + 1, 10))
    if n.count == "zoned":   # PIC 9(1)
        if u > 0.95:
            return (b"x" if ascii else b"\xab"), None    # no digit: null
        return (bytes([0x30 + v]) if ascii else bytes([0xF0 + v])), v
    if n.count == "comp":    # PIC 9(4) COMP: never null; 300 is far out of range
        if u > 0.95:
            v = 300
        return v.to_bytes(2, "big"), v
    assert n.count == "comp3"   # PIC 9(3) COMP-3: two bytes, 0 0 v sign
    if u > 0.9:
        return bytes([0x00, v << 4 | 0x0A]), None        # a sign nibble that is none: null
    return bytes([0x00, v << 4 | 0x0F]), v


COUNT_PIC = {"zoned": ("PIC 9(1)", 1), "comp": ("PIC 9(4) COMP", 2), "comp3": ("PIC 9(3) COMP-3", 2), "str": ("PIC X(2)", 2)}


def count_node(name: str, kind: str, count_max: int) -> Node:
    pic, size = COUNT_PIC[kind]
    return Node(name, pic, size, count=kind, count_max=count_max)


def emit_record(body: List[Node], rng, var_size: bool, ascii: bool = False, segs: Tuple[str, ...] = ("A", "B")) -> bytes:
    """One whole record of the layout, as extractRecord would lay it out: with variable_size_occurs an
    array takes the room of its present elements, without it the room of its maximum.  A segment id
    field draws the record's segment from `segs`; of the segment redefines (the record's last
    statements) the active one is emitted."""
    out = bytearray()
    deps: Dict[str, object] = {}

    def elements(n: Node) -> int:
        lo, hi = n.occurs
        if lo is None:
            return hi
        v = deps.get(n.dep)
        if isinstance(v, str):
            v = n.handlers.get(v)
        return v if v is not None and lo <= v <= hi else hi

    def one(n: Node, live: bool):
        if n.children is not None:
            many(n.children, live)
        elif n.count == "seg":
            deps["segment id"] = segs[int(rng.integers(0, len(segs)))]
            out.extend(_ebcdic_or_ascii(deps["segment id"], ascii))
        elif n.count:
            b, v = draw_count(rng, n, ascii)
            if live and v is not None:
                deps[n.name] = v
            out.extend(b)
        else:
            out.extend(n.gen(rng))

    def many(nodes: List[Node], live: bool):
        for n in nodes:
            if n.seg is not None:
                if deps.get("segment id") != n.seg:
                    continue
            elif n.redefines:    # overlays the statement before it (same size, nothing data-dependent)
                continue
            if n.occurs:
                k = elements(n) if live else 0
                for i in range(k if var_size else n.occurs[1]):
                    one(n, live and i < k)   # elements past the count are never decoded
            else:
                one(n, live)

    many(body, True)
    return bytes(out)


def records(body: List[Node], n: int, seed: int, var_size: bool = True, ascii: bool = False,
            whole: float = WHOLE_SHARE, segs: Tuple[str, ...] = ("A", "B")) -> List[bytes]:
    """n records; `whole` of them as emitted, the others cut at a uniform length in 1..length.  A record's
    length is its true length: what an RDW header says, or where the next record starts."""
    return records_and_full(body, n, seed, var_size, ascii, whole, segs)[0]


def records_and_full(body, n, seed, var_size=True, ascii=False, whole=WHOLE_SHARE, segs=("A", "B")):
    """(records, the length each had before it was cut)."""
    rng = np.random.default_rng(seed)
    recs, full = [], []
    for _ in range(n):
        b = emit_record(body, rng, var_size, ascii, segs)
        full.append(len(b))
        if rng.random() >= whole:
            b = b[:int(rng.integers(1, len(b) + 1))]
        recs.append(b)
    return recs, full


def rdw(recs: List[bytes]) -> bytes:
    return b"".join(bytes([0, 0, len(r) & 0xFF, len(r) >> 8]) + r for r in recs)


# ------------------------------------------------------------------------------------------------
# wrappers of the decoder slices
# ------------------------------------------------------------------------------------------------
_LINE = re.compile(r"\s+05\s+(\S+)\s+(.*)\.\s*$")


@functools.lru_cache(maxsize=None)
def slice_nodes(sid: str) -> Tuple[Node, ...]:
    """The slice's fields as nodes: the field lines as they are, the fuzz's byte generators."""
    ascii = S.SLICE_TABLE[sid][0] == "ascii"
    out = []
    for ln in S.field_lines(S.slice_text(sid)):
        name, pic = _LINE.match(ln).groups()
        p = S.leaves(S.parse(S.HEADER + ln + "\n", ascii))[0]
        assert p.name == name
        gen = (lambda rng, p=p: _random_ascii_bytes(rng, p, p.data_size, True)) if ascii else \
            (lambda rng, p=p: _random_bytes(rng, p, p.data_size))
        out.append(Node(name, pic, p.data_size, gen))
    return tuple(out)


def _pad_byte(ascii: bool):
    return (lambda rng: bytes([int(rng.integers(0x20, 0x7F))])) if ascii else \
        (lambda rng: bytes([int(rng.integers(0, 256))]))


def _tail() -> Node:
    def gen(rng):   # seven digits and a sign nibble
        d = [int(x) for x in rng.integers(0, 10, 7)]
        return bytes([d[0] << 4 | d[1], d[2] << 4 | d[3], d[4] << 4 | d[5], d[6] << 4 | (0x0C if rng.random() < 0.5 else 0x0D)])
    return Node("TAIL", "PIC S9(7) COMP-3", 4, gen)


def wrap(sid: str, how: str) -> List[Node]:
    """behind: the slice's fields behind an ODO array of 0..3 pad bytes (every alignment mod 4);
    inside: as the elements of an ODO array of groups; fixed: that array inside an outer fixed OCCURS,
    its dependee an element's field (variable_size_occurs = false: fixed-length records)."""
    ascii = S.SLICE_TABLE[sid][0] == "ascii"
    fields = list(slice_nodes(sid))
    if how == "behind":
        return [count_node("N-PAD", "zoned", 3),
                Node("PAD", "PIC X(1)", 1, _pad_byte(ascii), occurs=(0, 3), dep="N-PAD"), *fields, _tail()]
    els = [count_node("N-EL", "zoned", 2), Node("ELS", children=fields, occurs=(0, 2), dep="N-EL")]
    if how == "inside":
        return [*els, _tail()]
    assert how == "fixed"
    return [Node("OUTER", children=els, occurs=(None, 2)), _tail()]


# PAD's second element is null only in a record cut to one byte: the seeds that miss that moved on
SEED_BUMP: Dict[Tuple[str, str], int] = {("a4", "behind"): 3, ("f2", "behind"): 3}


def wrapped_seed(sid: str, how: str) -> int:
    return 7 * sum(map(ord, sid)) + WRAPPERS.index(how) + 1000 * SEED_BUMP.get((sid, how), 0)


@functools.lru_cache(maxsize=None)
def _wrapped(sid: str, how: str, n: int):
    body = wrap(sid, how)
    ascii = S.SLICE_TABLE[sid][0] == "ascii"
    return body, records(body, n, wrapped_seed(sid, how), var_size=how != "fixed", ascii=ascii,
                         whole=1.0 if how == "fixed" else WHOLE_SHARE)


def wrapped_records(sid: str, how: str, n: int = N_REC):
    """(layout, record list): `how` fixed gives whole records of one length."""
    body, recs = _wrapped(sid, how, n)
    return body, list(recs)


EBCDIC_OPTION = ("cp037", "both", "IBM")     # (code page, trim, float format)


def wrapper_parameters(sid: str, how: str, option=None, **kw):
    """ReaderParameters of a wrapped slice: option is a (code page, trim, float format) triple for an
    EBCDIC slice, the ascii_charset for an ASCII one."""
    from cobrix_amd.reader import ReaderParameters
    var = how != "fixed"
    if S.SLICE_TABLE[sid][0] == "ascii":
        enc = dict(is_ebcdic=False, ascii_charset=option or "")
    else:
        page, trim, fmt = option or EBCDIC_OPTION
        enc = dict(ebcdic_code_page=page, string_trimming_policy=trim, floating_point_format=fmt)
    return ReaderParameters(variable_size_occurs=var, is_record_sequence=var, **enc, **kw)


@functools.lru_cache(maxsize=None)
def can_be_malformed(sid: str, name: str) -> bool:
    """Whether the fuzz's bytes for the field ever decode to null (the oracle on 600 values of the field
    alone): a string and a binary integer never do."""
    from oracle import oracle as O
    if name == "TAIL" or name.startswith("N_"):
        return name == "N_EL"      # (draw_count's non-digit)
    ascii = S.SLICE_TABLE[sid][0] == "ascii"
    node = next(n for n in slice_nodes(sid) if n.name.replace("-", "_") == name)
    cb = S.parse(S.HEADER + f"           05  {name}  {node.pic}.\n", ascii, **({} if ascii else dict(code_page="cp037")))
    rng = np.random.default_rng(5)
    data = b"".join(node.gen(rng) for _ in range(600))
    return any(not r[2] for r in S.field_events(O.decode_fixed(cb, data))[name])


# ------------------------------------------------------------------------------------------------
# dense strings: PIC X(n), n = 1..13 and 24, behind PAD and inside ELS; bytes of all 256 values with
# the page's 2- and 3-byte entries over-weighted to half of all bytes
# ------------------------------------------------------------------------------------------------
DENSE_SIZES = tuple(range(1, 14)) + (24,)
DENSE_PAGES = ("cp875", "cp037", "windows-1252")     # the last as ASCII data (ascii_charset)
TRIMS = ("none", "left", "right", "both")


@functools.lru_cache(maxsize=None)
def multibyte(page: str) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """(bytes of 2 UTF-8 bytes, bytes of 3) of the page."""
    if page == "windows-1252":
        ln = [len(bytes([b]).decode("cp1252", errors="replace").encode("utf-8")) for b in range(256)]
    else:
        ln = [(e >> 24) & 3 for e in utf8_lut(lut_for(page))]
    return tuple(b for b in range(256) if ln[b] == 2), tuple(b for b in range(256) if ln[b] == 3)


DENSE_PLACES = ("behind", "inside")   # two layouts: one of 28 string fields took hipRTC over 6 s


def dense_layout(page: str, place: str) -> List[Node]:
    two, three = multibyte(page)
    assert two
    three = three or two       # cp037 has no 3-byte entry
    ascii = page == "windows-1252"
    blank = 0x20 if ascii else 0x40

    def gen(n):
        def g(rng):
            b = rng.integers(0, 256, n, dtype=np.uint8)
            u = rng.random(n)
            b = np.where(u < 0.25, rng.choice(two, n), b)
            b = np.where((u >= 0.25) & (u < 0.5), rng.choice(three, n), b).astype(np.uint8)
            v = rng.random()
            if v < 0.15:      # blanks at either end: the trims have work
                k = int(rng.integers(0, n + 1))
                b[:k] = blank
            elif v < 0.3:
                k = int(rng.integers(0, n + 1))
                b[n - k:] = blank
            elif v < 0.4:     # mostly single-byte values: short UTF-8 lengths from long fields
                b = np.where(rng.random(n) < 0.8, 0xC1 if not ascii else 0x41, b).astype(np.uint8)
            return b.tobytes()
        return g

    if place == "behind":
        return [count_node("N-PAD", "zoned", 3),
                Node("PAD", "PIC X(1)", 1, _pad_byte(ascii), occurs=(0, 3), dep="N-PAD"),
                *[Node(f"X{n:02d}", f"PIC X({n})", n, gen(n)) for n in DENSE_SIZES], _tail()]
    assert place == "inside"
    return [count_node("N-EL", "zoned", 2),
            Node("ELS", children=[Node(f"X{n:02d}", f"PIC X({n})", n, gen(n)) for n in DENSE_SIZES], occurs=(0, 2), dep="N-EL"),
            _tail()]


@functools.lru_cache(maxsize=None)
def _dense(page: str, place: str, n: int):
    body = dense_layout(page, place)
    return body, records(body, n, 1000 + 10 * DENSE_PAGES.index(page) + DENSE_PLACES.index(place), ascii=page == "windows-1252")


def dense_records(page: str, place: str, n: int = N_REC) -> Tuple[List[Node], List[bytes]]:
    body, recs = _dense(page, place, n)
    return body, list(recs)


def dense_parameters(page: str, trim: str, **kw):
    from cobrix_amd.reader import ReaderParameters
    enc = dict(is_ebcdic=False, ascii_charset=page) if page == "windows-1252" else dict(ebcdic_code_page=page)
    return ReaderParameters(variable_size_occurs=True, is_record_sequence=True, string_trimming_policy=trim, **enc, **kw)


# ------------------------------------------------------------------------------------------------
# random layouts
# ------------------------------------------------------------------------------------------------
FEATURES = ("odo_group", "odo_prim", "fixed_group", "fixed_prim", "min_count_1", "shared_dependee",
            "element_dependee", "dep_zoned", "dep_comp", "dep_comp3", "dep_comp3_null", "dep_string", "redefines",
            "filler", "segment_odo", "three_levels", "eight_names")
SEEDS = tuple(range(24))
PALETTE = ("PIC X(1)", "PIC X(3)", "PIC X(7)", "PIC X(12)", "PIC X(14)", "PIC 9(2)", "PIC S9(4)", "PIC S9(5)V99",
           "PIC 9(9)", "PIC S9(18)", "PIC S9(3) COMP-3", "PIC 9(9) COMP-3", "PIC S9(17) COMP-3", "PIC S9(4) COMP",
           "PIC 9(9) COMP", "PIC S9(18) COMP", "PIC S9(7)V99 COMP-3", "PIC 9(20) COMP-3", "COMP-2", "PIC S9(3)V9 COMP")
MAX_LEAVES, MAX_DEPTH, MAX_NAMES = 25, 4, 8


@functools.lru_cache(maxsize=None)
def _palette_prim(pic: str):
    return S.leaves(S.parse(S.HEADER + f"           05  P  {pic}.\n"))[0]


@dataclass
class Layout:
    seed: int
    body: List[Node]
    text: str
    options: Dict[str, object]        # ReaderParameters keywords besides the framing ones
    features: frozenset
    n_names: int
    segments: Tuple[str, ...]         # segment ids in the order of the segment redefines ("" none)

    def records(self, n: int, framed: bool, seed: int = 0) -> List[bytes]:
        """framed (RDW): 70 % whole records; not framed: whole records back to back, whose lengths
        VarOccursRecordExtractor has to find.  That extractor knows no segments: it walks A-PART without
        advancing and takes B-PART's walked size, so back to back every record is a B record (the RDW
        files hold both)."""
        return records(self.body, n, 100000 + 131 * self.seed + seed, whole=WHOLE_SHARE if framed else 1.0,
                       segs=("A", "B") if framed else ("B",))


def random_layout(seed: int, names: Optional[int] = None) -> Layout:
    """At most 4 nesting levels, 25 leaves and 8 DEPENDING ON names (`names`: that many; default: drawn,
    8 for every sixth seed).  A draw that ends above 25 leaves is drawn again."""
    for attempt in range(50):
        lay = _draw_layout(seed, names, attempt)
        if len(leaf_names(lay.body)) <= MAX_LEAVES:
            return lay
    raise AssertionError(f"seed {seed}: no layout within {MAX_LEAVES} leaves")


def _draw_layout(seed: int, names: Optional[int], attempt: int) -> Layout:
    rnd = random.Random(9176 + seed + 1000 * attempt)
    feats = set()
    uid = [0]
    leaves = [0]
    n_names = names if names is not None else (8 if seed % 6 == 0 else rnd.randint(1, 6))
    left = [n_names]

    def name(prefix: str) -> str:
        uid[0] += 1
        return f"{prefix}{uid[0]}"

    def leaf() -> Node:
        leaves[0] += 1
        pic = rnd.choice(PALETTE)
        p = _palette_prim(pic)
        return Node(name("F"), pic, p.data_size, lambda rng, p=p: _random_bytes(rng, p, p.data_size))

    def room() -> int:
        """Leaves still free: every name to come needs its dependee and one array leaf."""
        return MAX_LEAVES - leaves[0] - 2 * left[0]

    def some_leaves(k: int, need: int = 0, keep: int = 0) -> List[Node]:
        return [leaf() for _ in range(max(need, min(k, room() - keep)))]

    def odo(depth: int, in_element: bool) -> List[Node]:
        """A new dependee and the array(s) that use it."""
        left[0] -= 1
        kind = rnd.choice(["zoned", "zoned", "comp", "comp3", "str"])
        feats.add({"zoned": "dep_zoned", "comp": "dep_comp", "comp3": "dep_comp3", "str": "dep_string"}[kind])
        if kind == "comp3":
            feats.add("dep_comp3_null")
        hi = rnd.randint(2, 3)
        lo = 1 if rnd.random() < 0.3 else 0
        if lo:
            feats.add("min_count_1")
        dep = count_node(name("N"), kind, hi)
        leaves[0] += 1
        if in_element:
            feats.add("element_dependee")
        out = [dep]
        n_arrays = 2 if room() >= 3 and rnd.random() < 0.3 else 1
        if n_arrays == 2:
            feats.add("shared_dependee")
        if rnd.random() < 0.4:
            out += some_leaves(1, keep=n_arrays)          # the dependee need not sit next to its array
        for k in range(n_arrays):
            pending = n_arrays - k - 1    # this dependee's arrays still to come: a leaf each
            handlers = {"A": 0, "B": 1, "C": hi} if kind == "str" else {}
            if depth < MAX_DEPTH and rnd.random() < 0.7:
                feats.add("odo_group")
                kids = [leaf()] + some_leaves(rnd.randint(0, 2), keep=pending)
                if depth + 1 < MAX_DEPTH and left[0] > 0 and rnd.random() < 0.6:
                    kids += odo(depth + 1, True)
                    if depth + 1 >= 3:
                        feats.add("three_levels")
                elif depth + 1 < MAX_DEPTH and room() - pending >= 2 and rnd.random() < 0.3:
                    kids.append(fixed(depth + 1))
                arr = Node(name("G"), children=kids, occurs=(lo, hi), dep=dep.name, handlers=handlers)
            else:
                feats.add("odo_prim")
                arr = leaf()
                arr.occurs, arr.dep, arr.handlers = (lo, hi), dep.name, handlers
            out.append(arr)
            if k == 0 and n_arrays == 2:
                out += some_leaves(1, keep=pending)
        return out

    def fixed(depth: int) -> Node:
        """(costs at most two leaves)"""
        if depth < MAX_DEPTH and rnd.random() < 0.5:
            feats.add("fixed_group")
            return Node(name("G"), children=[leaf(), leaf()], occurs=(None, 2))
        feats.add("fixed_prim")
        n = leaf()
        n.occurs = (None, rnd.randint(2, 3))
        return n

    def redefine_pair() -> List[Node]:
        feats.add("redefines")
        leaves[0] += 3
        g = lambda rng: bytes(rng.integers(0, 256, 4, dtype=np.uint8))   # noqa: E731
        a = Node(name("G"), children=[Node(name("F"), "PIC X(4)", 4, g)])
        b = Node(name("G"), children=[Node(name("F"), "PIC S9(4) COMP", 2), Node(name("F"), "PIC 9(3) COMP-3", 2)],
                 redefines=a.name)
        return [a, b]

    def filler() -> Node:
        feats.add("filler")
        k = rnd.randint(1, 5)
        return Node("FILLER", f"PIC X({k})", k, lambda rng, k=k: bytes(rng.integers(0, 256, k, dtype=np.uint8)))

    segments: Tuple[str, ...] = ()
    use_segments = 2 <= n_names < 8 and rnd.random() < 0.5
    if use_segments:
        left[0] -= 2
        leaves[0] += 5      # SEG, two dependees, two arrays
    body: List[Node] = some_leaves(rnd.randint(1, 2), need=1)
    extras = [(redefine_pair, 3)] * (rnd.random() < 0.5) + [(filler, 0)] * (rnd.random() < 0.5) + \
             [(lambda: fixed(1), 2)] * (rnd.random() < 0.5)
    while left[0] > 0 or extras:
        if left[0] > 0:
            body += odo(1, False)
        if extras and (left[0] == 0 or rnd.random() < 0.6):
            make, cost = extras.pop()
            if room() >= cost:
                x = make()
                body += x if isinstance(x, list) else [x]
        if rnd.random() < 0.5:
            body += some_leaves(1)
    if use_segments:
        # as SEGODO: two segment redefines, each with its own dependee and ODO array, at the record's end
        feats.add("segment_odo")
        feats.update(("dep_zoned", "odo_prim"))
        sg = Node("SEG", "PIC X(1)", 1, count="seg")
        na, nb = count_node(name("N"), "zoned", 3), count_node(name("N"), "zoned", 2)
        pa, pb = _palette_prim("PIC S9(3) COMP-3"), _palette_prim("PIC X(4)")
        a = Node("A-PART", children=[na, Node(name("F"), "PIC S9(3) COMP-3", 2, lambda rng: _random_bytes(rng, pa, 2),
                                               occurs=(0, 3), dep=na.name)], seg="A")
        b = Node("B-PART", children=[nb, Node(name("F"), "PIC X(4)", 4, lambda rng: _random_bytes(rng, pb, 4),
                                               occurs=(0, 2), dep=nb.name)], redefines="A-PART", seg="B")
        body = [sg] + body + [a, b]
        segments = ("A", "B")
    if n_names == 8:
        feats.add("eight_names")
    options: Dict[str, object] = dict(variable_size_occurs=True, ebcdic_code_page="cp037")
    om = occurs_mappings(body)
    if om:
        options["occurs_mappings"] = om
    if segments:
        options.update(segment_field="SEG", segment_id_redefine_map={"A": "A_PART", "B": "B_PART"})
    return Layout(seed, body, copybook_text(body), options, frozenset(feats), n_names, segments)


def leaf_events(res) -> Dict[str, list]:
    """Per leaf name: (record, slot, valid, heap bytes of a valid string | None) of every value event, in
    record order (as staging_cases.field_events, for layouts whose leaves may be OCCURS themselves)."""
    from oracle import oracle as O
    ev = res.events
    vals = ev[ev["kind"] == O.EV_VALUE]
    out: Dict[str, list] = {}
    for p in S.leaves(res.ast.cb):
        v = vals[vals["node"] == res.ast.node_of(p)]
        v = v[np.argsort(v["rec"], kind="stable")]
        rows = []
        for e in v:
            valid = not e["isnull"]
            lo, hi = int(e["lo"]), int(e["hi"])
            rows.append((int(e["rec"]), int(e["slot"]), valid, res.heap[lo:lo + hi] if valid and p.is_string else None))
        out[p.name] = rows
    return out
