"""A minimal ctypes binding of the HIP runtime for the stream-contract tests (test infrastructure, no torch, no oracle).

It binds the runtime image that libspf_hip itself has loaded — the path `/proc/self/maps` shows for the libamdhip64 the
library's own handle resolves to — never a second copy: a stream created here must be a stream of the runtime that launches
the kernels.

`Stream` is a caller's `hipStreamNonBlocking` stream.  `Stream.gate()` enqueues a host function (`hipLaunchHostFunc`) that
waits on a `threading.Event`: everything enqueued behind it stays queued, the GPU idle, until the test opens the gate.  The
wait is capped at `CAP_S` seconds; the cap is a safety limit, not a measurement: `Stream.release()` fails when the cap, and
not the test, opened a gate.  `streams()` opens every gate, synchronizes and destroys the stream in a `finally`."""
import contextlib
import ctypes as C
import threading

import numpy as np

HIP_SUCCESS = 0
HIP_ERROR_NOT_READY = 600
STREAM_NON_BLOCKING = 1
EVENT_DISABLE_TIMING = 2
MEMCPY_DEVICE_TO_HOST = 2
MEMCPY_DEVICE_TO_DEVICE = 3
CAP_S = 10.0
# Copies of a few KiB run as kernels on a hardware queue, and the runtime deals its few hardware queues (GPU_MAX_HW_QUEUES) to
# the streams in turn: such a copy on ANOTHER stream can land on the queue of a gated stream and wait behind the gate (measured:
# 96 B and 4 KiB copies — device to device, to pinned and to pageable memory — waited out the cap; 48 KiB and 1 MiB did not).
# Large copies go through the copy engines, which no gate holds: `Stream.read` always moves at least MIN_READ bytes into
# pinned memory, so a buffer that is read while a gate is closed is allocated with at least `MIN_READ` bytes.
MIN_READ = 256 << 10

HOST_FN = C.CFUNCTYPE(None, C.c_void_p)
_P, _SZ, _I, _U = C.c_void_p, C.c_size_t, C.c_int, C.c_uint
_PROTOTYPES = [
    ("hipStreamCreateWithFlags", [C.POINTER(_P), _U]),
    ("hipStreamDestroy", [_P]),
    ("hipStreamQuery", [_P]),
    ("hipStreamSynchronize", [_P]),
    ("hipMemcpyAsync", [_P, _P, _SZ, _I, _P]),
    ("hipEventCreateWithFlags", [C.POINTER(_P), _U]),
    ("hipEventRecord", [_P, _P]),
    ("hipStreamWaitEvent", [_P, _P, _U]),
    ("hipEventDestroy", [_P]),
    ("hipLaunchHostFunc", [_P, HOST_FN, _P]),
    ("hipHostMalloc", [C.POINTER(_P), _SZ, _U]),
    ("hipHostFree", [_P]),
]
_RT = None


def runtime_path() -> str:
    """The libamdhip64 image libspf_hip is bound to: the `/proc/self/maps` entry that holds the address its own handle
    resolves a runtime symbol to.  (A process that also imported torch may have mapped a second copy of the runtime.)"""
    import spf_amd
    lib = spf_amd.load_library()
    addr = C.cast(lib.hipStreamSynchronize, _P).value
    with open("/proc/self/maps") as f:
        for line in f:
            fields = line.split(None, 5)
            lo, hi = (int(x, 16) for x in fields[0].split("-"))
            if lo <= addr < hi and len(fields) == 6 and "libamdhip64" in fields[5]:
                return fields[5].strip()
    raise RuntimeError("libspf_hip does not resolve hipStreamSynchronize to a mapped libamdhip64 image")


def runtime():
    global _RT
    if _RT is None:
        rt = C.CDLL(runtime_path())   # the path of a loaded image: dlopen returns that image
        for name, args in _PROTOTYPES:
            fn = getattr(rt, name)
            fn.restype, fn.argtypes = _I, args
        rt.hipGetErrorString.restype, rt.hipGetErrorString.argtypes = C.c_char_p, [_I]
        _RT = rt
    return _RT


def check(status: int, what: str):
    if status != HIP_SUCCESS:
        raise RuntimeError(f"{what}: HIP error {status} ({(runtime().hipGetErrorString(status) or b'').decode()})")


_PINNED = [_P(), 0]


def reserve_pinned(nbytes: int):
    """One pinned staging buffer for the process, grown HERE only: hipHostFree waits for the device, so a test reserves what it
    will read before it closes a gate."""
    nbytes = max(nbytes, MIN_READ)
    if _PINNED[1] < nbytes:
        if _PINNED[0]:
            check(runtime().hipHostFree(_PINNED[0]), "hipHostFree")
        _PINNED[0], _PINNED[1] = _P(), 0
        check(runtime().hipHostMalloc(C.byref(_PINNED[0]), nbytes, 0), "hipHostMalloc")
        _PINNED[1] = nbytes
    return _PINNED[0]


class Gate:
    """a host function on a stream that waits until `open()`; `capped` says the CAP_S limit ended the wait instead"""

    def __init__(self, stream: "Stream"):
        self._event = threading.Event()
        self.capped = False

        def wait(_user_data):
            self.capped = not self._event.wait(CAP_S)

        self._callback = HOST_FN(wait)   # the stream keeps `self`, hence the callback object, alive as long as it exists
        check(runtime().hipLaunchHostFunc(stream.handle, self._callback, None), "hipLaunchHostFunc")

    def open(self):
        self._event.set()


class Event:
    def __init__(self):
        self.handle = _P()
        check(runtime().hipEventCreateWithFlags(C.byref(self.handle), EVENT_DISABLE_TIMING), "hipEventCreateWithFlags")

    def record(self, stream: "Stream"):
        check(runtime().hipEventRecord(self.handle, stream.handle), "hipEventRecord")

    def destroy(self):
        if self.handle:
            check(runtime().hipEventDestroy(self.handle), "hipEventDestroy")
            self.handle = _P()


class Stream:
    """a caller's own non-blocking stream"""

    def __init__(self):
        self.handle = _P()
        self.gates = []
        check(runtime().hipStreamCreateWithFlags(C.byref(self.handle), STREAM_NON_BLOCKING), "hipStreamCreateWithFlags")

    def gate(self) -> Gate:
        g = Gate(self)
        self.gates.append(g)
        return g

    def busy(self) -> bool:
        """hipStreamQuery: True = hipErrorNotReady (work is queued or running), False = idle"""
        st = runtime().hipStreamQuery(self.handle)
        if st not in (HIP_SUCCESS, HIP_ERROR_NOT_READY):
            check(st, "hipStreamQuery")
        return st == HIP_ERROR_NOT_READY

    def synchronize(self):
        check(runtime().hipStreamSynchronize(self.handle), "hipStreamSynchronize")

    def copy(self, dst: int, src: int, nbytes: int):
        """device to device, asynchronous on this stream"""
        check(runtime().hipMemcpyAsync(dst, src, nbytes, MEMCPY_DEVICE_TO_DEVICE, self.handle), "hipMemcpyAsync (D2D)")

    def read(self, src: int, host: np.ndarray) -> np.ndarray:
        """device to host on this stream, then wait for this stream only.  The device buffer is at least MIN_READ bytes long."""
        assert host.flags.c_contiguous and host.flags.writeable
        n = max(host.nbytes, MIN_READ)
        assert _PINNED[1] >= n, "reserve_pinned() before the gate is closed"
        staging = _PINNED[0]
        check(runtime().hipMemcpyAsync(staging, src, n, MEMCPY_DEVICE_TO_HOST, self.handle), "hipMemcpyAsync (D2H)")
        self.synchronize()
        C.memmove(host.ctypes.data_as(_P), staging, host.nbytes)
        return host

    def wait_event(self, event: Event):
        check(runtime().hipStreamWaitEvent(self.handle, event.handle, 0), "hipStreamWaitEvent")

    def release(self):
        """open every gate, wait for the stream; the case is void when the cap opened a gate before the test did"""
        for g in self.gates:
            g.open()
        self.synchronize()
        assert not any(g.capped for g in self.gates), f"a gate was opened by its {CAP_S:.0f} s cap, not by the test"

    def close(self):
        if not self.handle:
            return
        try:
            for g in self.gates:
                g.open()
            runtime().hipStreamSynchronize(self.handle)
        finally:
            st = runtime().hipStreamDestroy(self.handle)
            self.handle = _P()
            self.gates = []
        check(st, "hipStreamDestroy")


@contextlib.contextmanager
def streams(n: int = 1):
    """n fresh non-blocking streams; whatever happens inside, every gate is opened and every stream synchronized and destroyed"""
    made = []
    try:
        for _ in range(n):
            made.append(Stream())
        yield made
    finally:
        for s in made:      # open every gate first: a stream may wait for an event of another
            for g in s.gates:
                g.open()
        for s in made:
            s.close()
