"""Status table of fp_plan_validate over mutated ops, host only (no GPU): what the validator answers is behaviour, and which
status wins when an op breaks several rules at once is part of it.  Two libraries that give the same table validate alike.

The corpus is every distinct fp_op (by its raw bytes) that the cases and variants of tools/plan_digest.py and the one-op plans
of tests/generic_op_cases.py emit, each kept with the weight count and arena size of the first plan it came from.  For every
op, with one fp_plan_validate call on a one-op array per entry:
  * the unmutated op's status (0) and fp_op_kernel_name;
  * the smallest weight_floats and the smallest arena_floats at which it still validates (bisection: the status is monotone
    in both limits), which pins every span expression exactly;
  * single mutations: every field set to old-1, old+1, old+2, old+4, 0, -1, 2*old and 1<<30 (values the field cannot hold
    and values equal to the old one are skipped); `flags` also with each of its low 9 bits toggled, `kind` also 0 .. 21;
  * COMPOUND compound mutations of two or three fields, drawn from the same value sets by a generator seeded from the op's
    bytes: only an op with two faults shows which check comes first.  At most one field of a compound takes 1<<30 (a second
    one takes the next value of its set): two dimensions that agree with each other at 2^30 pass the consistency checks and
    reach launchers whose int products then overflow, e.g. H = OH = 2^30 on a BLAZEBLOCK makes OH * OW wrap to 0 and
    fp_make_divisor(0) raise SIGFPE -- undefined behaviour in the launchers, nothing a status table can hold.

usage: python tools/validate_digest.py [--lib PATH] [--out FILE] [--compare FILE] [--only SUBSTRING]
  --lib PATH      validate with this libfacepath.so (another checkout's) instead of the package's; the plans are emitted by
                  this tree either way
  --out FILE      write the whole table as JSON
  --compare FILE  compare with a table written earlier; names every differing (op, mutation, old, new) and exits 1 if any
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from face_detection_and_recognition_amd import _lib as L  # noqa: E402
from tools.plan_digest import KIND, cases, switched, variants  # noqa: E402

SEED = 20240607
COMPOUND = 100
FIELDS = [name for name, _ in L.FpOp._fields_]
BITS = {name: 8 * ctypes.sizeof(t) for name, t in L.FpOp._fields_}
STATUS_CHARS = {0: "0", -1: "1", -2: "2", -3: "3", -4: "4", -5: "5"}


def bind(path=None):
    """The two entry points of a libfacepath.so: the package's own, or the one at `path`."""
    if path is None:
        return L.load()
    L.load()   # the HIP runtime the package binds to, first
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in ("fp_plan_validate", "fp_op_kernel_name"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = L.SIGNATURES[name]
    return lib


def values(name, old):
    """The values a single mutation gives field `name` of an op where it holds `old`, in a fixed order."""
    cand = [old - 1, old + 1, old + 2, old + 4, 0, -1, 2 * old, 1 << 30]
    if name == "flags":
        cand += [old ^ (1 << b) for b in range(9)]
    if name == "kind":
        cand += list(range(22))
    lim = 1 << (BITS[name] - 1)
    out = []
    for v in cand:
        if -lim <= v < lim and v != old and v not in out:
            out.append(v)
    return out


def compounds(raw, op):
    """[((field, value), ...)]: COMPOUND mutations of two or three distinct fields of the op whose bytes are `raw`."""
    draws = np.random.default_rng([SEED, zlib.crc32(raw)]).integers(0, 1 << 31, size=(COMPOUND, 7)).tolist()
    cand = {name: values(name, getattr(op, name)) for name in FIELDS}
    out = []
    for d in draws:
        names = []
        for j in range(2 + d[0] % 2):
            i = d[1 + j] % len(FIELDS)
            while FIELDS[i] in names:
                i = (i + 1) % len(FIELDS)
            names.append(FIELDS[i])
        parts = []
        for j, n in enumerate(names):
            k = d[4 + j] % len(cand[n])
            if cand[n][k] == 1 << 30 and any(v == 1 << 30 for _, v in parts):
                k = (k + 1) % len(cand[n])
            parts.append((n, cand[n][k]))
        out.append(tuple(parts))
    return out


def tight(validate, p, limits, which):
    """Smallest limits[which] at which the op still validates (the other limit as the plan has it)."""
    lo, hi = -1, limits[which]          # fails at lo (or lo = -1), validates at hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        trial = list(limits)
        trial[which] = mid
        if validate(p, 1, *trial) == 0:
            hi = mid
        else:
            lo = mid
    return hi


def record(lib, raw, n_weights, n_arena):
    """One op's row of the table; `multi` counts the compound mutations more than one part of which fails alone."""
    validate = lib.fp_plan_validate
    op = L.FpOp.from_buffer_copy(raw)
    p = ctypes.pointer(op)
    limits = (n_weights, n_arena)
    status = validate(p, 1, *limits)
    row = {"op": raw.hex(), "weights": n_weights, "arena": n_arena, "status": status,
           "kernel": lib.fp_op_kernel_name(p).decode()}
    row["tight"] = [tight(validate, p, limits, 0), tight(validate, p, limits, 1)] if status == 0 else None
    alone = {}
    for name in FIELDS:
        old = getattr(op, name)
        for v in values(name, old):
            setattr(op, name, v)
            alone[name, v] = validate(p, 1, *limits)
        setattr(op, name, old)
    row["single"] = "".join(STATUS_CHARS[s] for s in alone.values())
    out, multi = [], 0
    for parts in compounds(raw, op):
        for name, v in parts:
            setattr(op, name, v)
        out.append(STATUS_CHARS[validate(p, 1, *limits)])
        ctypes.memmove(p, raw, len(raw))
        multi += sum(alone[part] != 0 for part in parts) > 1
    row["compound"] = "".join(out)
    row["multi"] = multi
    return row


def labels(raw):
    """The mutations of an op in the order of its row: singles, then compounds."""
    op = L.FpOp.from_buffer_copy(raw)
    single = [f"{name}: {getattr(op, name)} -> {v}" for name in FIELDS for v in values(name, getattr(op, name))]
    return single, [", ".join(f"{n}: {getattr(op, n)} -> {v}" for n, v in parts) for parts in compounds(raw, op)]


def add_plan(corpus, pb):
    ops, weights, arena = pb.finish()
    for op in ops:
        corpus.setdefault(bytes(op), (int(weights.size), int(arena)))


def generic_corpus(corpus):
    import generic_op_cases as G
    for c in G.cases():
        add_plan(corpus, G.build(c)[0])


def group_of(raw):
    op = L.FpOp.from_buffer_copy(raw)
    return f"{KIND.get(op.kind, op.kind)}/{'SPLIT3' if op.flags & L.OPF_SPLIT3 else 'fp32'}"


def table(lib, corpus):
    """{group: [row]}: rows of one (kind, SPLIT3 or fp32) group in the order of their ops' bytes."""
    out = {}
    for raw in sorted(corpus):
        out.setdefault(group_of(raw), []).append(record(lib, raw, *corpus[raw]))
    return out


def summary(tab):
    """Per group: ops, calls, a SHA-256 over every status and kernel name in order, the status histogram, and of the tight
    extents a SHA-256 and the largest of each."""
    out = {}
    for group, rows in sorted(tab.items()):
        h, ht = hashlib.sha256(), hashlib.sha256()
        hist = {}
        for r in rows:
            text = f"{r['status']}|{r['kernel']}|{r['single']}|{r['compound']}\n"
            h.update(text.encode())
            ht.update(f"{r['tight']}\n".encode())
            for ch in r["single"] + r["compound"]:
                hist[ch] = hist.get(ch, 0) + 1
        out[group] = {"ops": len(rows), "calls": sum(hist.values()), "sha256": h.hexdigest(),
                      "histogram": {str(-int(ch)): n for ch, n in sorted(hist.items())},
                      "tight_sha256": ht.hexdigest(),
                      "tight_max": [max((r["tight"] or (-1, -1))[i] for r in rows) for i in (0, 1)],
                      "multi_fault_compounds": sum(r["multi"] for r in rows)}
    return out


def compare(want, got):
    """Print every difference between two tables; returns their number."""
    n = 0
    old = {r["op"]: r for rows in want.values() for r in rows}
    new = {r["op"]: r for rows in got.values() for r in rows}
    for key in sorted(set(old) | set(new)):
        a, b = old.get(key), new.get(key)
        if a is None or b is None:
            print(f"DIFFERS: op {key[:24]}... only in the {'new' if a is None else 'old'} table")
            n += 1
            continue
        what = f"{group_of(bytes.fromhex(key))} {b['kernel']} op {key[:24]}..."
        for field in ("status", "kernel", "tight"):
            if a[field] != b[field]:
                print(f"DIFFERS: {what} {field}: {a[field]} -> {b[field]}")
                n += 1
        single, compound = labels(bytes.fromhex(key))
        for field, names in (("single", single), ("compound", compound)):
            for i, (x, y) in enumerate(zip(a[field], b[field])):
                if x != y:
                    print(f"DIFFERS: {what} [{names[i]}]: -{x} -> -{y}")
                    n += 1
    return n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib")
    ap.add_argument("--out")
    ap.add_argument("--compare")
    ap.add_argument("--only", default="", help="emit only the plan_digest cases whose name contains this")
    args = ap.parse_args()
    lib = bind(args.lib)
    corpus = {}
    for name, classes, extra, emit in cases():
        if args.only not in name:
            continue
        for _, settings in variants(classes, extra):
            with switched(settings):
                add_plan(corpus, emit())
    generic_corpus(corpus)
    tab = table(lib, corpus)
    total = {}
    for group, s in summary(tab).items():
        print(f"{s['sha256'][:16]}  ops={s['ops']:5d}  calls={s['calls']:8d}  multi-fault={s['multi_fault_compounds']:7d}  "
              f"{s['histogram']}  {group}")
        for k, v in s["histogram"].items():
            total[k] = total.get(k, 0) + v
    rows = [r for g in tab.values() for r in g]
    print(f"{len(rows)} distinct ops of {len({group_of(k).split('/')[0] for k in corpus})} kinds, {sum(total.values())} "
          f"mutation calls, statuses {total}, {sum(r['multi'] for r in rows)} of {COMPOUND * len(rows)} compound mutations "
          f"with more than one fault, {sum(r['status'] != 0 for r in rows)} ops fail unmutated")
    rc = 1 if any(r["status"] != 0 for r in rows) else 0
    if args.out:
        with open(args.out, "w") as f:
            json.dump(tab, f)
    if args.compare:
        with open(args.compare) as f:
            want = json.load(f)
        if args.only:
            have = {r["op"] for g in tab.values() for r in g}
            want = {g: [r for r in rows if r["op"] in have] for g, rows in want.items()}
        n = compare(want, tab)
        print(f"{n} differences from {args.compare}")
        rc = rc or (1 if n else 0)
    return rc


if __name__ == "__main__":
    sys.exit(main())
