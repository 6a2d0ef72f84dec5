"""Red zones around memory that a test hands to the library: a payload of exactly the documented size inside one allocation, with a
poisoned zone in front of it and one behind it.  A call that writes a little past either end of what it was given changes a zone; a call
that reads a little past the end meets the poison instead of the allocator's stale zeros; a call that changes an input it calls read-only
changes the payload.  All three are assertions here (tests/test_zones_cpu.py proves on the CPU that each bites, and only where it should).

    Zoned(nbytes, shift=0, fill=0xA5, zone=1 << 20, device="cuda")      one torch.uint8 tensor of zone + shift + nbytes + zone bytes
    HostZoned(nbytes, shift=0, fill=0xA5, zone=1 << 20)                 the same in a numpy array, for the library's host outputs

The front zone is a multiple of 256 bytes and the tensor's own start is aligned at least that far (torch's allocators give 512 bytes on
the device, 64 on the host; the constructor checks 256 on the device and 64 on the host), so `shift` alone is the payload's alignment.

What this cannot see: an access farther than `zone` bytes from the payload.  The default of 1 MiB on each side spans what a workgroup of
any sweep kernel covers per grid stride (KDB_*_WG_BINS x 8 bytes is at most 8 KiB) and a thousand 1 KiB pages of the scatter paths; a
write that misses the payload by more than that -- a wrong base pointer, an index multiplied by the wrong stride -- lands outside the
tensor and is not observed.  Nor does a zone see a read that leaves no trace in the result (a value read and then masked off).

The rule for every test that uses these: no pointer or length handed to the library may leave the allocation.  The zones turn a small
overrun of the library's into a failed assertion; they are never the room for an access the test itself asks for outside its payload
-- with one exception that stays inside the tensor, the bite cases, which pass nbins + 1 on purpose so that the extra entry lies in the
back zone."""
import numpy as np

ZONE = 1 << 20


def _first_changed(zone_bytes, fill):
    """(offset, value) of the first byte of a zone that is not `fill`, or None; zone_bytes: a 1-d uint8 tensor or array"""
    bad = zone_bytes != fill
    if not bool(bad.any()):
        return None
    if isinstance(zone_bytes, np.ndarray):
        at = int(np.flatnonzero(bad)[0])
    else:
        at = int(bad.to("cpu").numpy().nonzero()[0][0])
    return at, int(zone_bytes[at])


class _Zones:
    """what Zoned and HostZoned share: the geometry and the three checks; a subclass provides self.buf (1-d uint8 of the whole
    allocation) and _copy(x)"""

    def _layout(self, nbytes, shift, fill, zone):
        if zone <= 0 or zone % 256:
            raise ValueError("the zone must be a positive multiple of 256 bytes")
        if nbytes < 0 or shift < 0 or not 0 <= fill <= 255:
            raise ValueError("nbytes, shift >= 0 and a byte to fill with")
        self.nbytes, self.shift, self.fill, self.zone = int(nbytes), int(shift), int(fill), int(zone)
        self.start = self.zone + self.shift                       # of the payload, in the allocation
        self.total = self.start + self.nbytes + self.zone
        self._snap = None

    @property
    def payload(self):
        return self.buf[self.start:self.start + self.nbytes]

    @property
    def front(self):
        return self.buf[:self.start]

    @property
    def back(self):
        return self.buf[self.start + self.nbytes:]

    def snapshot(self):
        self._snap = self._copy(self.payload)
        return self

    def refill_zones(self, fill=None):
        """poison both zones again (with another byte, if given): the payload stays"""
        if fill is not None:
            self.fill = int(fill)
        self.front[:] = self.fill
        self.back[:] = self.fill
        return self

    def assert_zones(self, where=""):
        found = []
        for name, z, base in (("front", self.front, -self.start), ("back", self.back, self.nbytes)):
            hit = _first_changed(z, self.fill)
            if hit is not None:
                found.append("%s zone: byte %d of it (%+d from the payload's start) holds 0x%02X, not 0x%02X"
                             % (name, hit[0], base + hit[0], hit[1], self.fill))
        assert not found, "%s: written outside the %d bytes handed over -- %s" % (where, self.nbytes, "; ".join(found))

    def assert_payload_unchanged(self, where=""):
        assert self._snap is not None, "no snapshot taken"
        hit = _first_changed(self.payload ^ self._snap, 0)
        assert hit is None, "%s: byte %d of the %d-byte payload changed (by 0x%02X)" % (where, hit[0], self.nbytes, hit[1])

    def assert_clean(self, where=""):
        self.assert_payload_unchanged(where)
        self.assert_zones(where)


class Zoned(_Zones):
    """a payload between two poisoned zones in one torch.uint8 tensor (see the module's docstring)"""

    def __init__(self, nbytes, shift=0, fill=0xA5, zone=ZONE, device="cuda"):
        import torch
        self._layout(nbytes, shift, fill, zone)
        self.device = torch.device(device)
        self.buf = torch.full((self.total,), self.fill, dtype=torch.uint8, device=self.device)
        need = 256 if self.device.type == "cuda" else 64
        assert self.buf.data_ptr() % need == 0, "the allocator's alignment is below %d bytes" % need

    @staticmethod
    def _copy(x):
        return x.clone()

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.start

    def view(self, dtype):
        """the payload as a tensor of `dtype` (nbytes must divide, and for the element size to be the alignment, so must shift)"""
        return self.payload.view(dtype)

    def write(self, array):
        """the payload := the bytes of a numpy array of exactly nbytes; the snapshot is taken too"""
        import torch
        raw = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
        assert raw.size == self.nbytes, "%d bytes for a payload of %d" % (raw.size, self.nbytes)
        self.payload.copy_(torch.from_numpy(raw.copy()))
        return self.snapshot()

    def zero(self):
        self.payload.zero_()
        return self.snapshot()

    def read(self, dtype=np.uint8):
        """the payload, as a numpy array on the host"""
        return self.payload.to("cpu").numpy().copy().view(dtype)

    def sync(self):
        if self.device.type == "cuda":
            import torch
            torch.cuda.synchronize(self.device)


class HostZoned(_Zones):
    """the same around a numpy output array: `array(dtype)` is what the library is given, `cap` entries and no more"""

    def __init__(self, nbytes, shift=0, fill=0xA5, zone=ZONE):
        self._layout(nbytes, shift, fill, zone)
        raw = np.empty(self.total + 64, dtype=np.uint8)
        skip = -raw.ctypes.data % 64
        self.buf = raw[skip:skip + self.total]
        self.buf[:] = self.fill

    @staticmethod
    def _copy(x):
        return x.copy()

    @property
    def ptr(self):
        return self.buf.ctypes.data + self.start

    def view(self, dtype):
        return self.payload.view(dtype)

    array = view

    def write(self, array):
        raw = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
        assert raw.size == self.nbytes, "%d bytes for a payload of %d" % (raw.size, self.nbytes)
        self.payload[:] = raw
        return self.snapshot()

    def read(self, dtype=np.uint8):
        return self.payload.copy().view(dtype)


def zoned_words(values, shift=0, fill=0xA5, zone=ZONE, device="cuda"):
    """a Zoned holding a uint64 vector"""
    values = np.ascontiguousarray(values, dtype=np.uint64)
    return Zoned(values.size * 8, shift=shift, fill=fill, zone=zone, device=device).write(values)


# ---------------------------------------------------------------------------------------------------------------
# the reuse contract of the host submits: a driver that poisons what the engine said it was done with
# ---------------------------------------------------------------------------------------------------------------
def drive_submit_poisoned(eng, batches, continues=None):
    """kdb_submit's promise -- "the caller's buffers may be reused as soon as it returns": every batch (bases, offsets) is copied into
    arrays of the driver's own, submitted, and both arrays are overwritten -- residues with 0xFF, offsets with all ones -- the moment the
    call is back.  `eng` needs submit(bases, offsets, continues=False); the caller then calls finish() and compares with the oracle.
    An engine that still reads the caller's memory after submit returned sees 0xFF (no residue) or offsets of 2^64 - 1."""
    for i, (bases, offsets) in enumerate(batches):
        b = np.array(bases, dtype=np.uint8, copy=True)
        o = np.array(offsets, dtype=np.uint64, copy=True)
        if continues is not None and continues[i]:
            eng.submit(b, o, continues=True)
        else:
            eng.submit(b, o)
        b[:] = 0xFF
        o[:] = np.uint64(0xFFFFFFFFFFFFFFFF)


def drive_pinned_ring_poisoned(eng, batches, ring):
    """kdb_submit_pinned's promise: a buffer is free once two further calls have returned, the offsets at once.  `ring`: three uint8
    arrays (pinned, on the device path), each as long as the longest batch.  Call N uses ring[N % 3]; when it has returned, the buffer
    of call N - 2 -- the one call N + 1 will use -- is filled with 0xFF and then loaded for call N + 1, and the offsets array of call N
    is overwritten with all ones.  This is the cycle parse._feed_file runs with the reader's ring of three."""
    assert len(ring) == 3
    n = len(batches)
    loaded = {}

    def load(i):
        b = batches[i][0]
        buf = ring[i % 3]
        buf[:] = 0xFF                                              # (call i - 3's residues, if it is still reading them, are gone now)
        buf[:b.size] = b
        loaded[i] = buf[:b.size]

    load(0)
    for i in range(n):
        o = np.array(batches[i][1], dtype=np.uint64, copy=True)
        eng.submit_pinned(loaded.pop(i), o)
        o[:] = np.uint64(0xFFFFFFFFFFFFFFFF)
        if i + 1 < n:
            load(i + 1)                                            # ring[(i + 1) % 3] is call i - 2's buffer: two calls have returned since
