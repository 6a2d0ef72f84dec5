"""CPU: that tests/zones.py bites where it should and nowhere else -- each of its three checks fails on exactly the byte it guards, an
untouched allocation passes all of them -- and that the drivers of the reuse contract (kdb_submit, kdb_submit_pinned) fail a stand-in
engine that keeps a reference to the caller's arrays instead of copying them.  No GPU: device="cpu" and the oracle."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zones  # noqa: E402

SMALL = 4096                                           # zone size of these tests: the geometry does not depend on it

CASES = [(64, 0), (64, 8), (37, 0), (37, 8), (1, 8), (0, 0)]


def _make(kind, nbytes, shift):
    if kind == "device":
        return zones.Zoned(nbytes, shift=shift, zone=SMALL, device="cpu")
    return zones.HostZoned(nbytes, shift=shift, zone=SMALL)


def _checks(z):
    """-> the names of the checks that fail"""
    failed = []
    for name, check in (("zones", z.assert_zones), ("payload", z.assert_payload_unchanged)):
        try:
            check("case")
        except AssertionError:
            failed.append(name)
    return failed


@pytest.mark.parametrize("kind", ["device", "host"])
@pytest.mark.parametrize("nbytes,shift", CASES)
def test_geometry_and_an_untouched_allocation_passes(kind, nbytes, shift):
    z = _make(kind, nbytes, shift)
    assert z.total == SMALL + shift + nbytes + SMALL
    assert z.ptr % 16 == shift % 16 and (z.ptr - shift) % 64 == 0          # shift alone sets the payload's alignment
    assert len(z.front) == SMALL + shift and len(z.back) == SMALL and len(z.payload) == nbytes
    z.write(np.arange(nbytes, dtype=np.uint8))
    assert z.read().tolist() == list(range(nbytes))
    assert _checks(z) == []
    z.assert_clean("untouched")


@pytest.mark.parametrize("kind", ["device", "host"])
@pytest.mark.parametrize("nbytes,shift", [c for c in CASES if c[0] > 0])
def test_each_check_fails_on_its_byte_and_only_it(kind, nbytes, shift):
    z = _make(kind, nbytes, shift)
    z.write(np.full(nbytes, 7, dtype=np.uint8))
    start = z.start
    for at, want in ((start - 1, ["zones"]),                               # the last byte of the front zone
                     (start + nbytes, ["zones"]),                          # the first byte of the back zone
                     (start + nbytes - 1, ["payload"]),                    # the last payload byte
                     (start, ["payload"])):                                # the first
        old = int(z.buf[at])
        z.buf[at] = old ^ 0x10
        assert _checks(z) == want, at
        z.buf[at] = old
        assert _checks(z) == []


def test_the_failure_names_the_first_changed_byte_of_each_zone():
    z = zones.Zoned(24, shift=8, zone=SMALL, device="cpu").zero()
    z.buf[z.start - 3] = 0x11
    z.buf[z.start - 1] = 0x22
    z.buf[z.start + 24 + 5] = 0x33
    with pytest.raises(AssertionError) as e:
        z.assert_zones("kdb_x")
    msg = str(e.value)
    assert "kdb_x" in msg and "(-3 from the payload's start) holds 0x11" in msg and "(+29 from the payload's start) holds 0x33" in msg
    assert "0x22" not in msg
    with pytest.raises(AssertionError, match="byte 2 of the 24-byte payload"):
        z.buf[z.start + 2] = 1
        z.assert_payload_unchanged("kdb_x")


def test_views_snapshots_and_other_fills():
    z = zones.zoned_words([1, 2, 2 ** 64 - 1], shift=8, fill=0x4E, zone=SMALL, device="cpu")
    assert z.nbytes == 24 and z.ptr % 16 == 8
    assert z.read(np.uint64).tolist() == [1, 2, 2 ** 64 - 1]
    import torch
    z.view(torch.int64)[1] = 5                                             # a view writes the payload itself
    with pytest.raises(AssertionError):
        z.assert_payload_unchanged("view")
    z.snapshot().assert_clean("after the snapshot")
    z.refill_zones(0xFF)
    assert int(z.buf[0]) == 0xFF and int(z.buf[-1]) == 0xFF
    z.assert_clean("refilled")
    assert z.read(np.uint64).tolist() == [1, 5, 2 ** 64 - 1]
    with pytest.raises(ValueError):
        zones.Zoned(8, zone=1000, device="cpu")                            # the front zone keeps the alignment: multiples of 256
    h = zones.HostZoned(5 * 8, zone=SMALL)
    out = h.array(np.uint64)
    out[:] = 9
    h.assert_zones("host")
    assert h.read(np.uint64).tolist() == [9] * 5


# ---- the reuse drivers against stand-in engines over the oracle ----

class _Standin:
    """submit / submit_pinned / finish over the oracle.  copies=True is what the contract asks of an engine; copies=False keeps a
    reference to the caller's arrays and reads them at finish -- an engine that reads the caller's memory late, always losing the race.
    ring_depth: how many submit_pinned calls back a buffer may still be read (2 is the contract)."""

    def __init__(self, oracle, k, copies, ring_depth=2):
        self.oracle, self.k, self.copies, self.depth = oracle, k, copies, ring_depth
        self.counts = np.zeros(4 ** k, dtype=np.uint64)
        self.total = 0
        self.held = []

    def _count(self, bases, offsets):
        if offsets.size < 2 or int(offsets[0]) != 0 or int(offsets[-1]) != bases.size or bool(np.any(np.diff(offsets.astype(np.int64)) < 0)):
            raise ValueError("offsets do not rise from 0 to the buffer's size")        # (what an engine would make of all ones)
        _, t = self.oracle.c_count(bases, offsets, self.k, True, self.oracle.N_DROP, counts=self.counts)
        self.total += t

    def submit(self, bases, offsets, continues=False):
        self.held.append((bases.copy(), offsets.copy()) if self.copies else (bases, offsets))

    def submit_pinned(self, bases, offsets):
        self.held.append((bases, offsets.copy() if self.copies else offsets))            # residues by reference: that is the call
        while len(self.held) > self.depth:                                               # call N waits for the copies of call N - depth
            self._count(*self.held.pop(0))

    def finish(self):
        for b, o in self.held:
            self._count(b, o)
        self.held = []
        return self.counts, self.total


def _batches(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        lens = rng.integers(20, 60, size=int(rng.integers(5, 12)))
        bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(lens.sum()))].copy()
        out.append((bases, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)))
    return out


def _want(oracle, batches, k):
    counts = np.zeros(4 ** k, dtype=np.uint64)
    total = 0
    for b, o in batches:
        total += oracle.c_count(b, o, k, True, oracle.N_DROP, counts=counts)[1]
    return counts, total


def _passes(drive, eng, want):
    """the poisoning check as the GPU tests make it: drive, finish, compare with the oracle"""
    try:
        drive(eng)
        counts, total = eng.finish()
    except Exception:  # noqa: BLE001 - garbage offsets or residues are a failure of the check, whatever the engine raises on them
        return False
    return total == want[1] and np.array_equal(counts, want[0])


def test_the_submit_driver_fails_an_engine_that_keeps_references(oracle):
    k, batches = 5, _batches(6, 1)
    want = _want(oracle, batches, k)
    good = _Standin(oracle, k, copies=True)
    drive = lambda eng: zones.drive_submit_poisoned(eng, batches)
    assert _passes(drive, good, want)
    lazy = _Standin(oracle, k, copies=False)
    assert not _passes(drive, lazy, want)
    assert all(int(b.max()) < 0xFF and int(o[0]) == 0 for b, o in batches)             # the driver poisons its own copies, never the cases


def test_the_pinned_ring_driver_allows_two_calls_of_delay_and_no_more(oracle):
    k, batches = 5, _batches(9, 2)
    want = _want(oracle, batches, k)
    size = max(b.size for b, _ in batches)
    drive = lambda eng: zones.drive_pinned_ring_poisoned(eng, batches, [np.zeros(size, dtype=np.uint8) for _ in range(3)])
    good = _Standin(oracle, k, copies=True, ring_depth=2)                  # reads a buffer until two further calls have returned: allowed
    assert _passes(drive, good, want)
    late = _Standin(oracle, k, copies=True, ring_depth=3)                  # one call later than promised
    assert not _passes(drive, late, want)
    lazy = _Standin(oracle, k, copies=False, ring_depth=2)                 # in time with the residues, but reads the offsets late
    assert not _passes(drive, lazy, want)
