"""A plain model of what include/kdbhip.h promises for an engine that lives through several batches, files and resets, a generator of
op sequences over that life, and a driver that runs a sequence on anything with kmerdb_amd.Engine's interface and checks every read
against the model.  No GPU and no torch at import: tests/test_lifecycle_model_cpu.py checks the model and the driver against an
oracle-backed stand-in, tests/test_gpu_lifecycle.py runs the same sequences on the real engine.

The engine carries host-side state from batch to batch (kdb_engine.hip, kdb_engine_options.hip.h, kdb_scatter_host.hip.h): whether the deferred histogram pass
may STORE a bucket's histogram over the vector or must ADD to it, batches pending in the page arena, records staged but not counted,
sticky error words.  None of it shows in a job that creates an engine, submits, reads once and closes; it shows in sequences."""
import numpy as np

KINDS = ("short", "bad_residue", "bad_layout", "not_uniform")
# what the engine's message says for each kind (kdb_engine.hip: check_errors); all four come up as ValueError
KIND_WORDS = {"short": "shorter than k", "bad_residue": "outside ACGTN", "bad_layout": "read_offsets must rise", "not_uniform": "records of one length"}
READ_OPS = ("finish", "table_stats", "finish_folded", "nullomers", "fold", "fold_into")       # ops that look at counts
LET = np.frombuffer(b"ACGTN", dtype=np.uint8)


class ModelError(Exception):
    """What the model raises where the engine must: .kind is one of KINDS, or 'sum' (kdb_finish: Sum(counts) != k-mers emitted)."""

    def __init__(self, kind):
        Exception.__init__(self, kind)
        self.kind = kind


def error_kind(exc):
    """The kind of an exception an engine raised: a stand-in says it outright, the real engine in its message."""
    kind = getattr(exc, "kind", None)
    if kind:
        return kind
    msg = str(exc)
    for kind, words in KIND_WORDS.items():
        if words in msg:
            return kind
    return "sum" if "Sum(" in msg else None


def pieces(record, k, cuts):
    """The byte pieces a caller hands to submit(..., continues=True) for one record cut behind residue cuts[0] <= cuts[1] <= ...:
    piece 0 = record[:cuts[0]]; piece j > 0 starts with the last k - 1 residues of what went before (include/kdbhip.h,
    KDB_SUBMIT_CONTINUES), so a window lies whole in exactly one piece.  Equal cuts give a piece of k - 1 residues (no new window)."""
    record = bytes(record)
    cuts = [int(c) for c in cuts]
    if not cuts or cuts != sorted(cuts) or cuts[0] < k or cuts[-1] >= len(record):
        raise ValueError("cuts must rise, piece 0 must hold k residues and the last piece at least one new one")
    ends = cuts + [len(record)]
    return [record[:ends[0]]] + [record[ends[j - 1] - (k - 1):ends[j]] for j in range(1, len(ends))]


class ModelEngine:
    """include/kdbhip.h in plain Python: the file vector as {id: count}, built from oracle.c_shred record by record."""

    def __init__(self, k, canon, n_mode, oracle):
        self.k, self.canon, self.n_mode, self.o = k, bool(canon), int(n_mode), oracle
        self.nbins = 4 ** k
        self.vec, self.acc = {}, {}
        self.emitted = 0
        self.folded_files = self.folded_total = 0
        self.poisoned = None

    # -- writes -----------------------------------------------------------------------------
    def _add(self, vec, ids):
        u, c = np.unique(np.asarray(ids, dtype=np.uint64), return_counts=True)
        for i, n in zip(u.tolist(), c.tolist()):
            vec[i] = vec.get(i, 0) + n

    def submit(self, records):
        omode = self.o.N_EXPAND if self.n_mode else self.o.N_DROP
        got = [self.o.c_shred(bytes(r), self.k, self.canon, omode)[0] for r in records]
        ids = np.concatenate(got) if got else np.zeros(0, np.uint64)
        self._add(self.vec, ids)
        self.emitted += int(ids.size)

    def submit_pieces(self, record, cuts):
        pieces(record, self.k, cuts)             # (the cuts must be ones a caller can make)
        self.submit([record])                    # the whole record, once

    def caller_adds(self, ids, n):
        """Somebody else adds n to bins `ids` of the vector (kdb_table handed its address out): the engine emitted nothing."""
        for i in ids:
            self.vec[int(i)] = self.vec.get(int(i), 0) + int(n)

    def submit_bad(self, kind):
        assert kind in KINDS
        if self.poisoned is None:
            self.poisoned = kind

    def reset(self):
        self.vec, self.acc = {}, {}
        self.emitted = 0
        self.folded_files = self.folded_total = 0
        self.poisoned = None

    # -- reads (every one raises the poisoned kind until reset) ----------------------------
    def _check(self):
        if self.poisoned:
            raise ModelError(self.poisoned)

    def sync(self):
        self._check()

    def table_stats(self):
        self._check()
        return dict(self.vec), sum(self.vec.values()), len(self.vec)

    def finish(self):
        self._check()
        if sum(self.vec.values()) != self.emitted:
            raise ModelError("sum")
        return dict(self.vec), self.emitted, len(self.vec)

    def fold_into(self, other):
        """-> (total, unique) of the file; its counts go to `other`'s accumulator, the file vector and its total start again."""
        self._check()
        if sum(self.vec.values()) != self.emitted:
            raise ModelError("sum")
        total, unique = self.emitted, len(self.vec)
        for i, n in self.vec.items():
            other.acc[i] = other.acc.get(i, 0) + n
        other.folded_files += 1
        other.folded_total += total
        self.vec, self.emitted = {}, 0
        return total, unique

    def fold(self):
        return self.fold_into(self)

    def finish_folded(self):
        self._check()
        return dict(self.acc), self.folded_total, len(self.acc)

    def nullomer_count(self, folded=False):
        self._check()
        return self.nbins - len(self.acc if folded else self.vec)


# ------------------------------------------------------------------------------------------------------------------------------
# sequences
# ------------------------------------------------------------------------------------------------------------------------------
# options a caller may change in the middle of a job: (name, values, applies at k)
MID_JOB_OPTIONS = (
    ("algo", (1, 2, 2), lambda k: True),
    ("defer_flush", (0, 1), lambda k: k >= 13),
    ("sc_lo_bits", (1, 3, 6, 9, 12, 14, 15, 0), lambda k: k >= 8),
    ("sc_grid", (1, 7, 64, 0), lambda k: True),
    ("sc_contig_pages", (0, 1), lambda k: k >= 8),
    ("one_level_max_k", (12, 13), lambda k: k == 13),
    ("arena_grow", (0, 1, 2), lambda k: k >= 13),
    ("arena_batches", (1, 2, 8), lambda k: k >= 13),
    ("smallk_old", (0, 1), lambda k: k <= 8),
)
OP_KINDS = ("submit_host", "submit_pinned", "submit_device", "submit_device_const", "pieces", "sync", "finish", "table_stats", "fold",
            "fold_into", "finish_folded", "nullomers", "nullomers_folded", "reset", "set_option", "bad")


def _records(rng, k, n, p_n, uniform=False):
    if uniform:
        lens = np.full(n, int(rng.integers(k, 301)))
    else:
        lens = rng.integers(k, 301, size=n)
    flat = LET[rng.choice(5, size=int(lens.sum()), p=[(1 - p_n) / 4] * 4 + [p_n])]
    ends = np.cumsum(lens)
    return [flat[int(e - l):int(e)].tobytes() for l, e in zip(lens, ends)]


def _bad_batch(rng, k, kind):
    """A batch of one kind of mistake among good records (device batches: records of one length, so that no kernel walks the offsets)."""
    if kind == "short":
        recs = _records(rng, k, 20, 0.0)
        recs[int(rng.integers(0, 20))] = b"ACGTACGTACGTACGTACGT"[:k - 1]
        return recs
    if kind == "bad_residue":
        recs = _records(rng, k, 20, 0.0)
        r = int(rng.integers(0, 20))
        recs[r] = recs[r][:-1] + b"X"
        return recs
    if kind == "bad_layout":
        return _records(rng, k, 20, 0.0, uniform=True)      # the driver hands its offsets over shifted by one
    recs = _records(rng, k, 20, 0.0, uniform=True)          # not_uniform: one record a residue longer
    recs[7] = recs[7] + b"A"
    return recs


def draw_sequence(rng, k, two_level_13=True):
    """-> list of ops (dicts with "op" in OP_KINDS) for one engine's life at this k.  Options that are locked once staging exists come
    first, as set_option ops with "init"; k = 13 takes the two-level path (one_level_max_k = 12) unless told otherwise."""
    ops = []
    expand = bool(rng.integers(0, 3) == 0)
    p_n = 0.002 if rng.integers(0, 2) else 0.0
    ops.append({"op": "create", "canon": bool(rng.integers(0, 2)), "n_mode": 1 if expand else 0})
    ops.append({"op": "set_option", "init": True, "name": "accum_bytes", "value": int(rng.choice([0, 0, 0, 1 << 20]))})
    if rng.integers(0, 3) == 0:
        ops.append({"op": "set_option", "init": True, "name": "stage_bytes", "value": int(rng.choice([4096, 65536]))})
        ops.append({"op": "set_option", "init": True, "name": "stage_reads", "value": int(rng.choice([3, 64, 4096]))})
    if k == 13 and two_level_13:
        ops.append({"op": "set_option", "init": True, "name": "one_level_max_k", "value": 12})
    algo = 2
    ops.append({"op": "set_option", "init": True, "name": "algo", "value": 2})
    copies = 0
    folded_self = False                       # (finish_folded / nullomers of the accumulator are a state error before the engine's first fold)

    def read(kind=None):
        nonlocal copies
        kind = kind or str(rng.choice(["finish", "finish", "table_stats", "nullomers"]))
        op = {"op": kind}
        if kind in ("finish", "table_stats", "finish_folded"):
            op["copy"] = bool(k < 13 or (copies < 3 and rng.integers(0, 3) == 0))
            copies += 1 if (op["copy"] and k >= 13) else 0
        ops.append(op)

    def submit(how=None, n=None):
        how = how or str(rng.choice(["submit_host", "submit_host", "submit_pinned", "submit_device", "submit_device_const"]))
        n = n or int(rng.choice([1, 7, 60, 200, 400]))
        ops.append({"op": how, "records": _records(rng, k, n, p_n, uniform=how == "submit_device_const")})

    def option(name=None, value=None):
        nonlocal algo
        if name is None:
            rows = [r for r in MID_JOB_OPTIONS if r[2](k)]
            name = rows[int(rng.integers(0, len(rows)))][0]
        if value is None:
            value = int(rng.choice([r[1] for r in MID_JOB_OPTIONS if r[0] == name][0]))
        if name == "algo":
            algo = value
        ops.append({"op": "set_option", "name": name, "value": int(value)})

    def pieces_op():
        rec = LET[rng.choice(5, size=int(rng.integers(5000, 40001)), p=[(1 - p_n) / 4] * 4 + [p_n])].tobytes()
        ncut = int(rng.integers(2, 6))
        cuts = sorted(int(c) for c in rng.integers(k, len(rec) - 1, size=ncut))
        if rng.integers(0, 2):
            cuts.insert(1, cuts[0] + int(rng.integers(0, 2)))           # a piece of k - 1 or of exactly k residues
        ops.append({"op": "pieces", "record": rec, "cuts": cuts, "pinned": bool(rng.integers(0, 2)),
                    "tail": _records(rng, k, int(rng.integers(1, 50)), p_n) if rng.integers(0, 2) else []})

    def bad():
        nonlocal algo
        kind = str(rng.choice(KINDS))
        submit("submit_host", 60)
        prev = algo
        if kind == "not_uniform" and algo != 1:
            option("algo", 1)                    # the direct-atomics kernel is the one that needs marks in the buffer
        ops.append({"op": "bad", "kind": kind, "records": _bad_batch(rng, k, kind)})
        if rng.integers(0, 2):
            submit("submit_host", 60)            # a later good batch does not erase it
        read()                                   # raises
        ops.append({"op": "reset"})
        if algo != prev:
            option("algo", prev)
        submit()
        read()

    # Building blocks, each an order of ops that exposes a flag left wrong; a sequence is a few of them one after the other.
    def block():
        nonlocal folded_self
        which = int(rng.integers(0, 11))
        if which == 0:                            # read -> submit -> read, no reset between
            submit(); read(); submit(); read()
        elif which == 1:                          # fold -> submit -> read
            how = str(rng.choice(["fold", "fold_into"]))
            folded_self = folded_self or how == "fold"
            submit(); ops.append({"op": how}); submit(); read()
            if folded_self:
                read("finish_folded")
        elif which == 2:                          # reset -> submit -> read
            submit(); ops.append({"op": "reset"}); submit(); read()
        elif which == 3:                          # direct atomics beside a pending batch
            submit("submit_host"); option("algo", 1); submit(); read("finish"); option("algo", 2)
        elif which == 4:                          # the bucket field moves under a pending batch
            submit("submit_host"); option("sc_lo_bits" if k >= 8 else "sc_grid"); read()
        elif which == 5:
            bad()
        elif which == 6:
            pieces_op(); read()
        elif which == 7:
            submit(); option(); submit(); ops.append({"op": "sync"}); option(); submit(); read()
        elif which == 8:
            folded_self = True
            submit(); ops.append({"op": "fold"}); ops.append({"op": "nullomers_folded"}); submit(); ops.append({"op": "fold"}); read("finish_folded")
        elif which == 9:
            submit(); submit(); read("table_stats"); ops.append({"op": "nullomers"})
        else:                                     # a reset clears the accumulator too
            folded_self = True
            submit(); ops.append({"op": "fold"}); ops.append({"op": "reset"}); read("finish_folded"); submit(); ops.append({"op": "fold"}); read("finish_folded")

    for _ in range(int(rng.integers(3, 6))):
        if rng.integers(0, 2):
            option()
        block()
    return ops


def pending_before(ops, k):
    """For each op: how many batches the two-level path holds in its page arena when the op begins, by the rules of kdb_engine.hip and
    kdb_engine_options.hip.h (None where the arena's size makes that unpredictable: arena_batches below its default).  A batch is pending
    after a submit at k > one_level_max_k under algo 2 with defer_flush 1 and no device-side accumulation of host submits; a sync, a read, a fold, a reset
    and a change of sc_lo_bits / one_level_max_k / defer_flush = 0 leave none."""
    opt = {"algo": 2, "defer_flush": 1, "one_level_max_k": 13, "accum_bytes": -1, "arena_batches": 8}
    small_stage = any(o["op"] == "set_option" and o["name"] in ("stage_bytes", "stage_reads") for o in ops)     # a submit is then many device batches
    out, pending, sure = [], 0, True
    for op in ops:
        out.append(pending if sure else None)
        what = op["op"]
        if what == "set_option":
            name, value = op["name"], op["value"]
            if name in ("sc_lo_bits", "one_level_max_k") or (name == "defer_flush" and not value):
                pending = 0
            if name == "arena_batches" and value < 8:
                sure = False
            if name in opt:
                opt[name] = value
        elif what in ("submit_host", "submit_pinned", "submit_device", "submit_device_const", "pieces", "bad"):
            host_fed = what in ("submit_host", "submit_pinned")
            staged = host_fed and (opt["accum_bytes"] > 0 or (opt["accum_bytes"] < 0 and k >= 13))
            if k > opt["one_level_max_k"] and opt["algo"] == 2 and opt["defer_flush"] and not staged:
                # (pieces: several device batches; a bad batch: not counted on; tiny staging buffers: a submit is many batches)
                pending = None if (pending is None or what in ("pieces", "bad") or (host_fed and small_stage)) else pending + 1
        elif what in ("sync", "reset", "fold", "fold_into", "nullomers", "nullomers_folded") or what in READ_OPS:
            pending = 0
    return out


def coverage(ops, k):
    """-> the set of ordered patterns (the issue's list) that this sequence holds.  'read' = finish / table_stats / nullomers."""
    reads = ("finish", "table_stats", "nullomers")
    submits = ("submit_host", "submit_pinned", "submit_device", "submit_device_const", "pieces")
    pend = pending_before(ops, k)
    kinds = [o["op"] for o in ops]
    have = set()

    def follows(i, *want):
        """ops after i, skipping set_option: do they begin with `want` (tuples of admissible kinds)?"""
        j = i + 1
        for w in want:
            while j < len(ops) and kinds[j] == "set_option":
                j += 1
            if j >= len(ops) or kinds[j] not in w:
                return False
            j += 1
        return True

    for i, op in enumerate(ops):
        what = kinds[i]
        if what in ("fold", "fold_into") and follows(i, submits, reads):
            have.add("fold,submit,read")
        if what == "reset" and follows(i, submits, reads):
            have.add("reset,submit,read")
        if what in reads and follows(i, submits, reads):
            have.add("read,submit,read")
        if what == "set_option" and not op.get("init") and pend[i]:
            if op["name"] == "algo" and op["value"] == 1 and follows(i, submits, reads):
                have.add("algo1 pending,submit,read")
            if op["name"] == "sc_lo_bits" and follows(i, reads):
                have.add("sc_lo_bits pending,read")
        if what == "bad" and follows(i, ("reset",), submits, reads):
            have.add("bad,reset,submit,read")
        if what == "bad" and follows(i, submits + reads, reads + ("reset",)):
            j = i + 1
            while j < len(ops) and kinds[j] != "reset":
                j += 1
            if j < len(ops) and follows(j, submits, reads):
                have.add("bad,reset,submit,read")
    return have


# the fixed seeds, (k, seed), that both test modules run; k = 13 goes through the two-level path (one_level_max_k = 12).
# tests/test_lifecycle_model_cpu.py asserts what they must contain: change them only together with a look at that test.
SEEDS = [(6, 14), (6, 16), (6, 28), (8, 6), (8, 11), (8, 34), (11, 10), (11, 23), (11, 30), (13, 4), (13, 5), (13, 24), (13, 31),
         (14, 2), (14, 12), (14, 13), (14, 31)]


def fixed_sequence(k, seed):
    return draw_sequence(np.random.Generator(np.random.PCG64(1000 * k + seed)), k)


PATTERNS = ("fold,submit,read", "reset,submit,read", "read,submit,read", "algo1 pending,submit,read", "sc_lo_bits pending,read",
            "bad,reset,submit,read")


# ------------------------------------------------------------------------------------------------------------------------------
# the driver
# ------------------------------------------------------------------------------------------------------------------------------
class GpuHost:
    """Where the driver gets device buffers, pinned memory and a writable view of the vector: torch and kmerdb_amd, imported at first use."""

    def to_device(self, arr):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda()
        return t, t.data_ptr()

    def pinned(self, nbytes):
        import kmerdb_amd
        return kmerdb_amd.pinned_empty(nbytes)

    def add_to_table(self, eng, ids, n):
        import torch
        t = eng.table_tensor()                    # (kdb_table: from here on the engine must assume that its vector is written behind its back)
        t[torch.as_tensor(np.asarray(ids, dtype=np.int64), device=t.device)] += int(n)
        torch.cuda.synchronize()


def pack(records):
    bases = np.frombuffer(b"".join(records), dtype=np.uint8).copy()
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in records])]).astype(np.uint64)
    return bases, offsets


def dense(vec, nbins):
    a = np.zeros(nbins, dtype=np.uint64)
    if vec:
        a[np.fromiter(vec.keys(), dtype=np.int64, count=len(vec))] = np.fromiter(vec.values(), dtype=np.uint64, count=len(vec))
    return a


def compare_vector(got, vec, nbins, got_sum):
    """Whole-vector equality of a host copy `got` with {id: count}.  Small vectors are compared bin by bin; a large one at the expected
    ids plus its Sum: the counters are unsigned, so expected ids equal and Sum equal to the expected total leaves every other bin zero."""
    if nbins <= 4 ** 12:
        return bool(np.array_equal(got, dense(vec, nbins)))
    ids = np.fromiter(vec.keys(), dtype=np.int64, count=len(vec))
    want = np.fromiter(vec.values(), dtype=np.uint64, count=len(vec))
    return bool(np.array_equal(got[ids], want)) and int(got_sum) == int(want.sum())


def submit_record_pieces(eng, host, k, record, cuts, tail=(), pinned=False, keep=None):
    """One record as continuation pieces; the last piece shares its submit call with the ordinary records `tail`."""
    ps = pieces(record, k, cuts)
    for j, p in enumerate(ps):
        recs = [p] + (list(tail) if j == len(ps) - 1 else [])
        bases, offsets = pack(recs)
        if pinned:
            buf = host.pinned(max(bases.size, 1))
            buf[:bases.size] = bases
            if keep is not None:
                keep.append(buf)
            eng.submit_pinned(buf[:bases.size], offsets, continues=j > 0)
        else:
            eng.submit(bases, offsets, continues=j > 0)


def run_sequence(engine_factory, ops, model, host=None, observe=None):
    """Run `ops` on engine_factory(canon, n_mode) engines and on `model` side by side; every read is compared, exactly.  -> the checks
    made, as (op index, what) pairs.  An engine-owned vector is read through finish() / table_stats() alone (never through
    table_tensor(): kdb_table would end the store form of the deferred histogram pass for the engine's life).  observe(i, op, engine)
    is called before every op."""
    host = host or GpuHost()
    checks, keep = [], []
    create = ops[0]
    assert create["op"] == "create"
    eng = engine_factory(create["canon"], create["n_mode"])
    other, other_model = None, None
    k, nbins = model.k, model.nbins

    def expect(i, what, ok, detail=""):
        assert ok, "op %d (%s): %s %s" % (i, ops[i]["op"], what, detail)
        checks.append((i, what))

    def raises(i, fn):
        try:
            fn()
        except Exception as e:  # noqa: BLE001 - the kind is what is checked
            expect(i, "raises " + model.poisoned, error_kind(e) == model.poisoned, "(got %s: %s)" % (type(e).__name__, e))
        else:
            expect(i, "raises " + model.poisoned, False, "(nothing raised)")

    try:
        for i, op in enumerate(ops[1:], start=1):
            what = op["op"]
            if observe is not None:
                observe(i, op, eng)
            if what == "set_option":
                eng.set_option(op["name"], op["value"])
            elif what in ("submit_host", "submit_pinned", "submit_device", "submit_device_const"):
                bases, offsets = pack(op["records"])
                if what == "submit_host":
                    eng.submit(bases, offsets)
                elif what == "submit_pinned":
                    buf = host.pinned(bases.size)
                    buf[:] = bases
                    keep.append(buf)
                    eng.submit_pinned(buf, offsets)
                else:
                    d_b, p_b = host.to_device(bases)
                    d_o, p_o = host.to_device(offsets)
                    keep.append((d_b, d_o))
                    (eng.submit_device if what == "submit_device" else eng.submit_device_const)(p_b, bases.size, p_o, len(offsets) - 1)
                model.submit(op["records"])
            elif what == "pieces":
                submit_record_pieces(eng, host, k, op["record"], op["cuts"], op["tail"], op["pinned"], keep)
                model.submit_pieces(op["record"], op["cuts"])
                model.submit(op["tail"])
            elif what == "bad":
                bases, offsets = pack(op["records"])
                if op["kind"] in ("short", "bad_residue"):
                    eng.submit(bases, offsets)
                else:
                    d_b, p_b = host.to_device(bases)
                    d_o, p_o = host.to_device(offsets + np.uint64(1) if op["kind"] == "bad_layout" else offsets)
                    keep.append((d_b, d_o))
                    (eng.submit_device if op["kind"] == "bad_layout" else eng.submit_device_const)(p_b, bases.size, p_o, len(offsets) - 1)
                model.submit_bad(op["kind"])
            elif what == "caller_adds":
                host.add_to_table(eng, op["ids"], op["n"])
                model.caller_adds(op["ids"], op["n"])
            elif what == "reset":
                eng.reset()
                model.reset()
                keep.clear()
            elif model.poisoned:                 # every read (and sync, and fold) raises the kind's error until reset
                into = None
                if what == "fold_into":
                    if other is None:
                        other, other_model = engine_factory(create["canon"], create["n_mode"]), ModelEngine(k, model.canon, model.n_mode, model.o)
                    into = other
                call = {"sync": eng.sync, "finish": lambda: eng.finish(copy=False), "table_stats": lambda: eng.table_stats(copy=False),
                        "finish_folded": lambda: eng.finish_folded(copy=False), "nullomers": lambda: eng.nullomers(),
                        "nullomers_folded": lambda: eng.nullomers(folded=True), "fold": eng.fold_file,
                        "fold_into": lambda: eng.fold_file(into=into)}[what]
                raises(i, call)
            elif what == "sync":
                eng.sync()
                keep.clear()
            elif what in ("finish", "table_stats", "finish_folded"):
                want_sum_error = False
                try:
                    vec, total, unique = getattr(model, what)()
                except ModelError as e:
                    assert e.kind == "sum"
                    want_sum_error = True
                if want_sum_error:
                    try:
                        getattr(eng, what)(copy=False)
                    except Exception as e:  # noqa: BLE001
                        expect(i, what + " raises sum", error_kind(e) == "sum", str(e))
                    else:
                        expect(i, what + " raises sum", False, "(nothing raised)")
                    continue
                got, g_total, g_unique = getattr(eng, what)(copy=bool(op.get("copy", True)))
                expect(i, what + " totals", (g_total, g_unique) == (total, unique), "got %r, want %r" % ((g_total, g_unique), (total, unique)))
                if got is not None:
                    expect(i, what + " vector", compare_vector(got, vec, nbins, g_total))
                    del got
                elif what != "finish_folded":
                    n0 = len(eng.nullomers()) if nbins <= 4 ** 8 else _nullomer_count(eng, False)
                    expect(i, what + " nullomer count", n0 == model.nullomer_count(False))
                keep.clear()
            elif what in ("nullomers", "nullomers_folded"):
                folded = what == "nullomers_folded"
                want = model.nullomer_count(folded)
                if nbins <= 4 ** 8:              # the ids themselves where the list is short
                    ids = eng.nullomers(folded=folded)
                    src = model.acc if folded else model.vec
                    expect(i, what + " ids", np.array_equal(ids, np.flatnonzero(dense(src, nbins) == 0).astype(np.uint64)))
                else:
                    expect(i, what + " count", _nullomer_count(eng, folded) == want)
                keep.clear()
            elif what in ("fold", "fold_into"):
                if what == "fold_into" and other is None:
                    other, other_model = engine_factory(create["canon"], create["n_mode"]), ModelEngine(k, model.canon, model.n_mode, model.o)
                try:
                    want = model.fold() if what == "fold" else model.fold_into(other_model)
                except ModelError as e:
                    raise AssertionError("op %d: a fold behind a caller's write is outside what the header promises (%s)" % (i, e.kind))
                got = eng.fold_file() if what == "fold" else eng.fold_file(into=other)
                expect(i, what + " totals", tuple(got) == tuple(want), "got %r, want %r" % (got, want))
                if what == "fold_into":
                    _, t2, u2 = other.finish_folded(copy=False)
                    expect(i, "fold_into accumulator totals", (t2, u2) == other_model.finish_folded()[1:])
                keep.clear()
            else:
                raise ValueError("unknown op %r" % what)
    finally:
        eng.close()
        if other is not None:
            other.close()
    return checks


def _nullomer_count(eng, folded):
    """The number alone (kdb_nullomers with ids_out = NULL): no list of 4^k ids comes back."""
    import ctypes
    c = ctypes.c_uint64(0)
    lib = getattr(eng, "_lib", None)
    if lib is None:
        return eng.nullomer_count(folded)        # (a stand-in)
    rc = lib.kdb_nullomers(eng._h, 1 if folded else 0, None, 0, ctypes.byref(c))
    if rc != 0:
        from kmerdb_amd import _abi
        _abi.check(rc)
    return c.value
