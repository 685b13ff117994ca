"""Host-side mirror of the reference's distributed-FFT API over the C-ABI (include/dfft.h).

Function names and argument meaning follow /root/reference/3dmpifft_opt/include/fft_mpi_3d_api.h:68-86 so that tests read
like the reference's driver (fftSpeed3d_c2c.cpp): fft_mpi_init -> fft_mpi_plan_dft_c2c_3d -> fft_mpi_execute_dft_3d_c2c ->
fft_mpi_destroy_plan.  torch is used only to own device memory and to select the device; all arithmetic happens in the
HIP kernels of libdfft_mi355x.so.  There is no CPU path here.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

from . import _lib as L
from ._lib import (BACKWARD, EXEC_ASYNC, EXEC_NO_TIMING, EXEC_PRINT, EXEC_SYNC_STAGES, F32, F64, FILTER_COMPLEX, FILTER_REAL, FORWARD, PLAN_ANY_LENGTH,  # noqa: F401
                   PLAN_DEFAULT, PLAN_INPUT_FROM_IN, PLAN_NATURAL, PLAN_OVERLAP, PLAN_UNFUSED, DfftError)


def _ll3(N: Sequence[int]):
    return (C.c_longlong * 3)(int(N[0]), int(N[1]), int(N[2]))


# ---- host-only slab bookkeeping (usable without a GPU) ------------------------------------------------------------------
def get_proper_device_num(N, ini_devices_in_rank: int, mpi_size: int, mpi_rank: int, real_devices: int = -1) -> Tuple[int, int]:
    """getProperDeviceNum, fft_mpi_3d_api.cpp:232-272 -> (newDeviceCount, newDeviceCountInNode)."""
    lib = L.load()
    tot, inr = C.c_int(), C.c_int()
    L.check(lib.dfft_proper_device_count(_ll3(N), ini_devices_in_rank, mpi_size, mpi_rank, real_devices, C.byref(tot),
                                         C.byref(inr)), "dfft_proper_device_count")
    return tot.value, inr.value


def get_data_count(N, total_devices: int, global_idx: int) -> int:
    """getDataCountForNode, fft_mpi_3d_api.cpp:274-287 (per device)."""
    return int(L.load().dfft_local_count(_ll3(N), total_devices, global_idx))


def get_max_data_count(n0: int, n1: int, n2: int, total_devices: int, is_last: bool) -> int:
    """getMaxDataCount, fft_mpi_3d_api.cpp:289-316."""
    return int(L.load().dfft_max_count(n0, n1, n2, total_devices, 1 if is_last else 0))


@dataclass
class ExchangeLayout:
    scount: List[int]
    soffset: List[int]
    rcount: List[int]
    roffset: List[int]


def exchange_layout(n0, n1, n2, total_devices: int, global_idx: int, direction: int) -> ExchangeLayout:
    """tInfo of fft_mpi_plan_dft_c2c_3d, fft_mpi_3d_api.cpp:84-133 (elements)."""
    lib = L.load()
    arrs = [(C.c_longlong * total_devices)() for _ in range(4)]
    L.check(lib.dfft_exchange_layout(n0, n1, n2, total_devices, global_idx, direction, *arrs), "dfft_exchange_layout")
    return ExchangeLayout(*[list(a) for a in arrs])


def exchange_part_layout(n0, n1, n2, total_devices: int, global_idx: int, part_planes: int, part: int, ycuts: int = 1,
                         ycut: int = -1, direction: int = FORWARD):
    """Messages of one piece of the overlapped exchange: list of (peer, soffset, scount, roffset, rcount)."""
    lib = L.load()
    cap = total_devices * max(1, ycuts)
    peer = (C.c_int * cap)()
    arrs = [(C.c_longlong * cap)() for _ in range(4)]
    n = lib.dfft_exchange_part_layout(n0, n1, n2, total_devices, global_idx, direction, part_planes, part, ycuts, ycut, cap,
                                      peer, *arrs)
    if n < 0:
        L.check(n, "dfft_exchange_part_layout")
    return [(peer[i], arrs[0][i], arrs[1][i], arrs[2][i], arrs[3][i]) for i in range(n)]


def local_size(n0, n1, n2, total_devices: int, global_idx: int) -> Tuple[int, int, int, int]:
    """(local_n0, local_0_start, local_n1, local_1_start) -- fft_mpi_local_size_3d (declared, fft_mpi_3d_api.h:73)."""
    lib = L.load()
    v = [C.c_longlong() for _ in range(4)]
    L.check(lib.dfft_local_size(n0, n1, n2, total_devices, global_idx, *[C.byref(x) for x in v]), "dfft_local_size")
    return tuple(int(x.value) for x in v)


def fft_mpi_init(N, ini_devices_in_rank: int, mpi_size: int = 1, mpi_rank: int = 0, real_devices: int = -1):
    """fft_mpi_init, fft_mpi_3d_api.cpp:3-39 -> (newDeviceCount, newDeviceCountInNode, dataCountInNode[])."""
    tot, inr = get_proper_device_num(N, ini_devices_in_rank, mpi_size, mpi_rank, real_devices)
    import math
    first = mpi_rank * math.ceil(tot / mpi_size)
    counts = [get_data_count(N, tot, first + i) for i in range(inr)]
    return tot, inr, counts


# ---- communicators -----------------------------------------------------------------------------------------------------
def device_pci_bus_id(device: int = -1) -> str:
    """PCI address of a HIP device (-1: the current one) -- dfft_device_pci_bus_id."""
    buf = C.create_string_buffer(64)
    L.check(L.load().dfft_device_pci_bus_id(device, buf, 64), "dfft_device_pci_bus_id")
    return buf.value.decode()


class Comm:
    def __init__(self, handle, kind: str, size: int):
        self.handle, self.kind, self.size = handle, kind, size

    @staticmethod
    def local(total_devices: int) -> "Comm":
        h = C.c_void_p()
        L.check(L.load().dfft_comm_create_local(total_devices, C.byref(h)), "dfft_comm_create_local")
        return Comm(h, "local", total_devices)

    @staticmethod
    def rccl_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        L.check(L.load().dfft_rccl_unique_id(buf), "dfft_rccl_unique_id")
        return buf.raw

    @staticmethod
    def rccl(unique_id: bytes, total_devices: int, global_idx: int) -> "Comm":
        assert len(unique_id) == 128
        h = C.c_void_p()
        L.check(L.load().dfft_comm_create_rccl(unique_id, total_devices, global_idx, C.byref(h)), "dfft_comm_create_rccl")
        return Comm(h, "rccl", total_devices)

    @staticmethod
    def ipc(total_devices: int, global_idx: int, async_exchange: bool = False) -> "Comm":
        """One process per device without RCCL: hipIpc-shared receive buffers, device-to-device pushes, barriers over the
        dfft_boot_* rendezvous (DFFT_RANK/... or torchrun's RANK/WORLD_SIZE/MASTER_ADDR/MASTER_PORT)."""
        h = C.c_void_p()
        L.check(L.load().dfft_comm_create_ipc(total_devices, global_idx, 1 if async_exchange else 0, C.byref(h)),
                "dfft_comm_create_ipc")
        return Comm(h, "ipc-async" if async_exchange else "ipc", total_devices)

    def info(self) -> dict:
        """{'kind', 'size', 'rank', 'device'} as the transport reports them (dfft_comm_info)."""
        k, s, r, d = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        L.check(L.load().dfft_comm_info(self.handle, C.byref(k), C.byref(s), C.byref(r), C.byref(d)), "dfft_comm_info")
        return {"kind": ("local", "rccl", "ipc", "ipc-async")[k.value], "size": s.value, "rank": r.value, "device": d.value}

    def destroy(self):
        if self.handle:
            L.load().dfft_comm_destroy(self.handle)
            self.handle = None


# ---- plans ----------------------------------------------------------------------------------------------------------------
def _dtype_code(t) -> int:
    import torch
    if t.dtype == torch.complex128:
        return F64
    if t.dtype == torch.complex64:
        return F32
    raise TypeError("dfft buffers must be torch.complex128 or torch.complex64 device tensors")


class Plan:
    """fft_mpi_3d_plan (fft_mpi_3d_api.h:11-66): owns bufferDev1; `in`/`out` tensors stay owned by the caller."""

    def __init__(self, n0, n1, n2, inp, out, comm: Optional[Comm], global_idx: int, total_devices: int, direction: int,
                 flags: int = PLAN_DEFAULT):
        import torch
        lib = L.load()
        if not inp.is_cuda:
            raise DfftError(L.ENOGPU, "Plan", "buffers must live on a HIP device (no CPU fallback)")
        self.N = (int(n0), int(n1), int(n2))
        self.dtype = _dtype_code(inp)
        self.direction = direction
        self.total_devices, self.global_idx = total_devices, global_idx
        self.max_count = get_max_data_count(n0, n1, n2, total_devices, global_idx == total_devices - 1)
        if inp.numel() < self.max_count or (out is not None and out.numel() < self.max_count):
            raise ValueError(f"in/out must hold getMaxDataCount = {self.max_count} elements")
        self._in, self._out, self._comm = inp, out, comm  # keep alive
        self.handle = C.c_void_p()
        torch.cuda.synchronize(inp.device)  # plan creation copies `in` with a blocking hipMemcpy on the null stream
        with torch.cuda.device(inp.device):
            L.check(lib.dfft_plan_create(C.byref(self.handle), n0, n1, n2, self.dtype, direction, inp.data_ptr(),
                                         out.data_ptr() if out is not None else None,
                                         comm.handle if comm is not None else None, global_idx, total_devices, flags),
                    "dfft_plan_create")
        self.device = inp.device

    @property
    def bufferDev1(self) -> int:
        return int(L.load().dfft_plan_buffer1(self.handle))

    @property
    def stream(self) -> int:
        return int(L.load().dfft_plan_stream(self.handle) or 0)

    def load_input(self, src) -> None:
        """hipMemcpy(plan->bufferDev1, data, ...) as the reference driver does (fftSpeed3d_c2c.cpp:78)."""
        import torch
        n = src.numel()
        assert n <= self.max_count and _dtype_code(src) == self.dtype
        view = self.buffer1_tensor(n)
        view.copy_(src.reshape(-1))
        torch.cuda.synchronize(self.device)

    def buffer1_tensor(self, count: Optional[int] = None):
        """A torch view of bufferDev1 (no copy), via __cuda_array_interface__."""
        import torch
        count = self.max_count if count is None else count
        tdtype = torch.complex128 if self.dtype == F64 else torch.complex64
        comp = "<c16" if self.dtype == F64 else "<c8"

        class _Raw:
            pass

        r = _Raw()
        r.__cuda_array_interface__ = {"shape": (count,), "typestr": comp, "data": (self.bufferDev1, False), "version": 2}
        t = torch.as_tensor(r, device=self.device)
        assert t.dtype == tdtype
        return t

    def execute(self, flags: int = EXEC_ASYNC) -> None:
        """fft_mpi_execute_dft_3d_c2c (fft_mpi_3d_api.cpp:181-214)."""
        import torch
        with torch.cuda.device(self.device):
            L.check(L.load().dfft_execute(self.handle, flags), "dfft_execute")

    def sync(self) -> None:
        L.check(L.load().dfft_plan_sync(self.handle), "dfft_plan_sync")

    def tune(self) -> None:
        """Plan-time measurement (dfft_plan_tune): times the X-pass kernel alone on a few candidate allocations of the plan's
        internal hand-over buffer and keeps the fastest; the probe launches leave garbage in the result buffer."""
        import torch
        with torch.cuda.device(self.device):
            L.check(L.load().dfft_plan_tune(self.handle), "dfft_plan_tune")

    def describe(self) -> str:
        """How this plan executes (dfft_plan_describe): pipeline, YZ stage form, chunk geometry, hand-over buffer, rotation."""
        buf = C.create_string_buffer(512)
        L.check(L.load().dfft_plan_describe(self.handle, buf, 512), "dfft_plan_describe")
        return buf.value.decode()

    def tune_report(self) -> dict:
        """{'candidates_ms': [...], 'kept': i, 'kept_retimed_ms': t} of the last tune() (dfft_plan_tune_report)."""
        ms = (C.c_double * 128)()
        kept, fin = C.c_int(-1), C.c_double(0.0)
        n = L.load().dfft_plan_tune_report(self.handle, 128, ms, C.byref(kept), C.byref(fin))
        if n < 0:
            L.check(n, "dfft_plan_tune_report")
        return {"candidates_ms": [round(ms[i], 4) for i in range(min(n, 128))], "kept": kept.value, "kept_retimed_ms": round(fin.value, 4)}

    def set_scale(self, s: float) -> None:
        """Multiply the result of every later execute by s (folded into the X-pass kernel; 1.0 = the reference's
        un-normalised transform)."""
        L.check(L.load().dfft_plan_set_scale(self.handle, float(s)), "dfft_plan_set_scale")

    def stage_times(self) -> List[float]:
        t = (C.c_double * 4)()
        L.check(L.load().dfft_stage_times(self.handle, t), "dfft_stage_times")
        return list(t)

    def kernel_times(self) -> List[float]:
        """Seconds spent in the Z-row, Y-column and X-column FFT kernels of the last ASYNC execute (HIP events)."""
        t = (C.c_double * 3)()
        L.check(L.load().dfft_kernel_times(self.handle, t), "dfft_kernel_times")
        return list(t)

    def destroy(self) -> None:
        """dfft_plan_destroy.  Its return code is the last place a failure of an execute nobody synchronised THROUGH THE LIBRARY can
        surface (a caller that waits with torch.cuda.synchronize() instead of sync()): raised here, after the handle is gone."""
        if self.handle:
            h, self.handle = self.handle, None
            L.check(L.load().dfft_plan_destroy(h), "dfft_plan_destroy")

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def r2c_counts(n0, n1, n2, total_devices: int, global_idx: int) -> Tuple[int, int]:
    """(reals, complex elements) the real-side / complex-side buffers of an r2c plan must hold on device global_idx (dfft_r2c_counts)."""
    lib = L.load()
    r, c = C.c_longlong(), C.c_longlong()
    L.check(lib.dfft_r2c_counts(n0, n1, n2, total_devices, global_idx, C.byref(r), C.byref(c)), "dfft_r2c_counts")
    return int(r.value), int(c.value)


_R2C_PAIRS = {"float64": "complex128", "float32": "complex64"}


class PlanR2C(Plan):
    """Real-to-complex (FORWARD) / complex-to-real (BACKWARD) slab plan (dfft_plan_create_r2c).  Real side: float64 / float32
    [x_local][N1][N2]; complex side: complex128 / complex64 [y_local][N2/2+1][N0].  FORWARD: inp real, out complex; BACKWARD: inp complex,
    out real.  Shares Plan's execute / sync / set_scale / stage_times / describe / destroy; bufferDev1 holds the real slab (FORWARD) or
    the bins (BACKWARD)."""

    def __init__(self, n0, n1, n2, inp, out, comm: Optional[Comm], global_idx: int, total_devices: int, direction: int,
                 flags: int = PLAN_DEFAULT, any_length: bool = False):
        import torch
        lib = L.load()
        if inp is None or out is None:
            raise ValueError("PlanR2C: real-to-complex plans are out of place (inp and out are both required)")
        if not inp.is_cuda or not out.is_cuda:
            raise DfftError(L.ENOGPU, "PlanR2C", "buffers must live on a HIP device (no CPU fallback)")
        if inp.device != out.device:
            raise ValueError(f"PlanR2C: inp is on {inp.device}, out on {out.device}")
        real, cplx = (inp, out) if direction == FORWARD else (out, inp)
        rname, cname = str(real.dtype).replace("torch.", ""), str(cplx.dtype).replace("torch.", "")
        if _R2C_PAIRS.get(rname) != cname:
            raise TypeError(f"PlanR2C: the real / complex buffers must be float64 / complex128 or float32 / complex64, got {rname} / {cname}")
        self.N = (int(n0), int(n1), int(n2))
        self.dtype = F64 if rname == "float64" else F32
        self.direction = direction
        self.total_devices, self.global_idx = total_devices, global_idx
        self.real_count, self.complex_count = r2c_counts(n0, n1, n2, total_devices, global_idx)
        if real.numel() < self.real_count or cplx.numel() < self.complex_count:
            raise ValueError(f"PlanR2C: the real buffer must hold {self.real_count} elements and the complex one {self.complex_count} "
                             f"(r2c_counts), got {real.numel()} / {cplx.numel()}")
        # bufferDev1 holds the input side
        self.max_count = self.real_count if direction == FORWARD else self.complex_count
        self._in, self._out, self._comm = inp, out, comm  # keep alive
        self.handle = C.c_void_p()
        torch.cuda.synchronize(inp.device)
        with torch.cuda.device(inp.device):
            # any_length: the real axis may be of any real_form != 0 (dfft_plan_create_r2c_any); otherwise dfft_plan_create_r2c's limits
            create, name = (lib.dfft_plan_create_r2c_any, "dfft_plan_create_r2c_any") if any_length else (lib.dfft_plan_create_r2c, "dfft_plan_create_r2c")
            L.check(create(C.byref(self.handle), n0, n1, n2, self.dtype, direction, inp.data_ptr(), out.data_ptr(),
                           comm.handle if comm is not None else None, global_idx, total_devices, flags), name)
        self.device = inp.device

    def load_input(self, src) -> None:
        """Copy the next input (real slab for FORWARD, bins for BACKWARD) into bufferDev1."""
        import torch
        view = self.buffer1_tensor(src.numel())
        assert src.numel() <= self.max_count and src.dtype == view.dtype
        view.copy_(src.reshape(-1))
        torch.cuda.synchronize(self.device)

    def buffer1_tensor(self, count: Optional[int] = None):
        """A torch view of bufferDev1 (no copy): real elements for FORWARD plans, complex ones for BACKWARD plans."""
        import torch
        count = self.max_count if count is None else count
        if self.direction == FORWARD:
            typestr, tdtype = ("<f8", torch.float64) if self.dtype == F64 else ("<f4", torch.float32)
        else:
            typestr, tdtype = ("<c16", torch.complex128) if self.dtype == F64 else ("<c8", torch.complex64)

        class _Raw:
            pass

        r = _Raw()
        r.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (self.bufferDev1, False), "version": 2}
        t = torch.as_tensor(r, device=self.device)
        assert t.dtype == tdtype
        return t


def conv_filter_count(n0, n1, n2, total_devices: int, global_idx: int) -> int:
    """Elements of device global_idx's share of a PlanConv filter: local_n1 * N2 * N0 (dfft_conv_filter_count)."""
    n = int(L.load().dfft_conv_filter_count(n0, n1, n2, total_devices, global_idx))
    if n < 0:
        raise ValueError("conv_filter_count: bad arguments")
    return n


class PlanConv(Plan):
    """Spectral-filter plan (dfft_plan_create_conv): y = ifftn(fftn(x) * H) with numpy's conventions, inp / out complex128 / complex64
    X slabs [x_local][N1][N2]; out None or inp: in place.  inp is read at every execute.  The filter is given with set_filter (its
    spectrum, in a forward Plan's output layout [y_local][N2][N0]; a real tensor selects the real-filter kernels) or set_kernel (a
    real-space kernel in the input layout).  Shares Plan's execute / sync / describe / stage_times / set_scale / destroy; set_scale takes
    effect at the next set_filter / set_kernel."""

    def __init__(self, n0, n1, n2, inp, out, comm: Optional[Comm], global_idx: int, total_devices: int, flags: int = PLAN_DEFAULT):
        import torch
        lib = L.load()
        if not inp.is_cuda:
            raise DfftError(L.ENOGPU, "PlanConv", "buffers must live on a HIP device (no CPU fallback)")
        self.N = (int(n0), int(n1), int(n2))
        self.dtype = _dtype_code(inp)
        self.direction = FORWARD
        self.total_devices, self.global_idx = total_devices, global_idx
        self.max_count = get_data_count(self.N, total_devices, global_idx)
        self.filter_count = conv_filter_count(n0, n1, n2, total_devices, global_idx)
        if inp.numel() < self.max_count or (out is not None and out.numel() < self.max_count):
            raise ValueError(f"in/out must hold getDataCount = {self.max_count} elements")
        if out is not None and out.dtype != inp.dtype:
            raise TypeError("PlanConv: inp and out must have the same dtype")
        self._in, self._out, self._comm = inp, out, comm  # keep alive
        self.handle = C.c_void_p()
        torch.cuda.synchronize(inp.device)
        with torch.cuda.device(inp.device):
            L.check(lib.dfft_plan_create_conv(C.byref(self.handle), n0, n1, n2, self.dtype, inp.data_ptr(),
                                              out.data_ptr() if out is not None else None,
                                              comm.handle if comm is not None else None, global_idx, total_devices, flags),
                    "dfft_plan_create_conv")
        self.device = inp.device

    def _check_operand(self, t, what: str, count: int, dtypes) -> None:
        """Argument checks of set_filter / set_kernel, made before the library is called."""
        cls = type(self).__name__
        if not hasattr(t, "dtype") or not hasattr(t, "is_contiguous"):
            raise TypeError(f"{cls}.{what}: a torch tensor is required")
        name = str(t.dtype).replace("torch.", "")
        if name not in dtypes:
            raise TypeError(f"{cls}.{what}: dtype {name} does not match the plan's precision (expected {' or '.join(dtypes)})")
        if t.numel() != count:
            raise ValueError(f"{cls}.{what}: {count} elements expected on this device, got {t.numel()}")
        if not t.is_contiguous():
            raise ValueError(f"{cls}.{what}: the tensor must be contiguous")
        if not t.is_cuda or t.device != self.device:
            raise ValueError(f"{cls}.{what}: the tensor must live on the plan's device {self.device}")

    def set_filter(self, h) -> None:
        """The filter's spectrum on this device, [y_local][N2][N0] (any shape with that many elements, C order): complex tensor of the
        plan's dtype, or a real tensor of the matching precision for a real filter.  The plan keeps a private copy."""
        import torch
        cplx, real = ("complex128", "float64") if self.dtype == F64 else ("complex64", "float32")
        self._check_operand(h, "set_filter", self.filter_count, (cplx, real))
        kind = FILTER_COMPLEX if h.is_complex() else FILTER_REAL
        with torch.cuda.device(self.device):
            L.check(L.load().dfft_conv_set_filter(self.handle, h.data_ptr(), kind), "dfft_conv_set_filter")

    def set_kernel(self, k) -> None:
        """The filter is fftn(k): k is a real-space kernel in the plan's input layout [x_local][N1][N2], complex dtype of the plan."""
        import torch
        self._check_operand(k, "set_kernel", self.max_count, ("complex128" if self.dtype == F64 else "complex64",))
        with torch.cuda.device(self.device):
            L.check(L.load().dfft_conv_set_kernel(self.handle, k.data_ptr()), "dfft_conv_set_kernel")

    def load_input(self, src) -> None:
        raise DfftError(L.EUNSUPPORTED, "PlanConv.load_input", "spectral-filter plans read `inp` at every execute")

    def buffer1_tensor(self, count: Optional[int] = None):
        raise DfftError(L.EUNSUPPORTED, "PlanConv.buffer1_tensor", "spectral-filter plans have no caller-visible bufferDev1")


def conv_real_filter_count(n0, n1, n2, total_devices: int, global_idx: int) -> int:
    """Elements of device global_idx's share of a PlanConvReal filter: local_n1 * (N2/2 + 1) * N0 (dfft_conv_real_filter_count)."""
    n = int(L.load().dfft_conv_real_filter_count(n0, n1, n2, total_devices, global_idx))
    if n < 0:
        raise ValueError("conv_real_filter_count: bad arguments")
    return n


class PlanConvReal(PlanConv):
    """Real-field spectral-filter plan (dfft_plan_create_conv_real): y = irfftn(rfftn(x) * H, s=(N0, N1, N2)) with numpy's conventions,
    inp / out float64 / float32 X slabs [x_local][N1][N2]; out None or inp: in place.  inp is read at every execute.  set_filter takes
    the filter's half spectrum in a forward PlanR2C's output layout [y_local][N2/2+1][N0] (complex of the matching precision, or a real
    tensor for a real filter), set_kernel a real-space kernel in the input layout (real dtype of the plan).  Everything else is
    PlanConv's; describe() reports the width of the plan's private spectrum as width=<Nc>."""

    def __init__(self, n0, n1, n2, inp, out, comm: Optional[Comm], global_idx: int, total_devices: int, flags: int = PLAN_DEFAULT):
        import torch
        lib = L.load()
        if not inp.is_cuda:
            raise DfftError(L.ENOGPU, "PlanConvReal", "buffers must live on a HIP device (no CPU fallback)")
        name = str(inp.dtype).replace("torch.", "")
        if name not in _R2C_PAIRS:
            raise TypeError(f"PlanConvReal: buffers must be torch.float64 or torch.float32 device tensors, got {name}")
        self.N = (int(n0), int(n1), int(n2))
        self.dtype = F64 if name == "float64" else F32
        self.direction = FORWARD
        self.total_devices, self.global_idx = total_devices, global_idx
        self.max_count = get_data_count(self.N, total_devices, global_idx)
        self.filter_count = conv_real_filter_count(n0, n1, n2, total_devices, global_idx)
        if inp.numel() < self.max_count or (out is not None and out.numel() < self.max_count):
            raise ValueError(f"in/out must hold getDataCount = {self.max_count} elements")
        if out is not None and out.dtype != inp.dtype:
            raise TypeError("PlanConvReal: inp and out must have the same dtype")
        if out is not None and out.device != inp.device:
            raise ValueError(f"PlanConvReal: inp is on {inp.device}, out on {out.device}")
        self._in, self._out, self._comm = inp, out, comm  # keep alive
        self.handle = C.c_void_p()
        torch.cuda.synchronize(inp.device)
        with torch.cuda.device(inp.device):
            L.check(lib.dfft_plan_create_conv_real(C.byref(self.handle), n0, n1, n2, self.dtype, inp.data_ptr(),
                                                   out.data_ptr() if out is not None else None,
                                                   comm.handle if comm is not None else None, global_idx, total_devices, flags),
                    "dfft_plan_create_conv_real")
        self.device = inp.device

    def set_kernel(self, k) -> None:
        """The filter is rfftn(k): k is a real-space kernel in the plan's input layout [x_local][N1][N2], real dtype of the plan."""
        import torch
        self._check_operand(k, "set_kernel", self.max_count, ("float64" if self.dtype == F64 else "float32",))
        with torch.cuda.device(self.device):
            L.check(L.load().dfft_conv_set_kernel(self.handle, k.data_ptr()), "dfft_conv_set_kernel")


class PlanConvRealMulti(PlanConvReal):
    """Multi-output real-field spectral-filter plan (dfft_plan_create_conv_real_multi): K real outputs of one real input,
    outs[k] = irfftn(rfftn(inp) * H * a_k[:, None, None] * b_k[None, :, None] * c_k[None, None, :], s=(N0, N1, N2)), with one base filter H
    (set_filter / set_kernel as for PlanConvReal) and per-output factors (set_factors; ones until set).  inp and every out: float64 /
    float32 X slabs [x_local][N1][N2]; one of outs may be inp.  The input is transformed once and the filter kept once; describe() reports
    pipeline=conv-real-multi outputs=<K>.  Everything else is PlanConvReal's."""

    def __init__(self, n0, n1, n2, inp, outs, comm: Optional[Comm], global_idx: int, total_devices: int, flags: int = PLAN_DEFAULT):
        import torch
        lib = L.load()
        outs = list(outs)
        if not inp.is_cuda:
            raise DfftError(L.ENOGPU, "PlanConvRealMulti", "buffers must live on a HIP device (no CPU fallback)")
        name = str(inp.dtype).replace("torch.", "")
        if name not in _R2C_PAIRS:
            raise TypeError(f"PlanConvRealMulti: buffers must be torch.float64 or torch.float32 device tensors, got {name}")
        if not 1 <= len(outs) <= L.CONV_MAX_OUTPUTS:
            raise ValueError(f"PlanConvRealMulti: 1 .. {L.CONV_MAX_OUTPUTS} outputs, got {len(outs)}")
        self.N = (int(n0), int(n1), int(n2))
        self.dtype = F64 if name == "float64" else F32
        self.direction = FORWARD
        self.total_devices, self.global_idx = total_devices, global_idx
        self.noutputs = len(outs)
        self.max_count = get_data_count(self.N, total_devices, global_idx)
        self.filter_count = conv_real_filter_count(n0, n1, n2, total_devices, global_idx)
        for o in outs:
            if o.dtype != inp.dtype:
                raise TypeError("PlanConvRealMulti: inp and every out must have the same dtype")
            if o.device != inp.device:
                raise ValueError(f"PlanConvRealMulti: inp is on {inp.device}, an out on {o.device}")
        if inp.numel() < self.max_count or any(o.numel() < self.max_count for o in outs):
            raise ValueError(f"in/outs must hold getDataCount = {self.max_count} elements")
        self._in, self._out, self._outs, self._comm = inp, outs[0], outs, comm  # keep alive
        self.handle = C.c_void_p()
        ptrs = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        torch.cuda.synchronize(inp.device)
        with torch.cuda.device(inp.device):
            L.check(lib.dfft_plan_create_conv_real_multi(C.byref(self.handle), n0, n1, n2, self.dtype, inp.data_ptr(), ptrs, len(outs),
                                                         comm.handle if comm is not None else None, global_idx, total_devices, flags),
                    "dfft_plan_create_conv_real_multi")
        self.device = inp.device

    def set_factors(self, k: int, ax=None, ay=None, az=None) -> None:
        """The separable factors of output k: device tensors of the plan's complex dtype with N0, N1 (the whole global vector) and N2/2 + 1
        elements; None: ones.  The plan keeps private copies; the other outputs are left alone."""
        import torch
        if not 0 <= int(k) < self.noutputs:
            raise ValueError(f"PlanConvRealMulti.set_factors: output {k} of {self.noutputs}")
        cplx = "complex128" if self.dtype == F64 else "complex64"
        for t, count in ((ax, self.N[0]), (ay, self.N[1]), (az, self.N[2] // 2 + 1)):
            if t is not None:
                self._check_operand(t, "set_factors", count, (cplx,))
        with torch.cuda.device(self.device):
            L.check(L.load().dfft_conv_set_factors(self.handle, int(k), *[t.data_ptr() if t is not None else None for t in (ax, ay, az)]),
                    "dfft_conv_set_factors")


def fft_mpi_plan_dft_c2c_3d(n0, n1, n2, inp, out, comm, global_idx, total_devices, direction, flags=PLAN_DEFAULT) -> Plan:
    return Plan(n0, n1, n2, inp, out, comm, global_idx, total_devices, direction, flags)


def fft_mpi_execute_dft_3d_c2c(plan: Plan, flags: int = EXEC_SYNC_STAGES) -> None:
    plan.execute(flags)
    plan.sync()


def fft_mpi_destroy_plan(plan: Plan) -> None:
    plan.destroy()


# ---- batched 1D building blocks ---------------------------------------------------------------------------------------------
def _check_out(x, out):
    """`out` (None: a fresh tensor) must have x's shape, dtype and device and be contiguous: the C entry points take bare pointers."""
    import torch
    if out is None:
        return torch.empty_like(x)
    assert out.shape == x.shape and out.dtype == x.dtype and out.device == x.device and out.is_contiguous(), \
        f"out must be a contiguous {x.dtype} tensor of shape {tuple(x.shape)} on {x.device}"
    return out


def fft1d_rows(x, direction: int = FORWARD, out=None):
    """Length-n FFT of every contiguous row of a (batch, n) complex device tensor."""
    import torch
    assert x.is_cuda and x.is_contiguous() and x.dim() == 2
    out = _check_out(x, out)
    with torch.cuda.device(x.device):
        L.check(L.load().dfft_fft1d_rows(x.data_ptr(), out.data_ptr(), x.shape[1], x.shape[0], _dtype_code(x), direction,
                                         None), "dfft_fft1d_rows")
        torch.cuda.synchronize()
    return out


def fft1d_cols(x, direction: int = FORWARD, out=None):
    """Length-n FFT down the columns of every (n, width) matrix of a (batch, n, width) complex device tensor."""
    import torch
    assert x.is_cuda and x.is_contiguous() and x.dim() == 3
    out = _check_out(x, out)
    with torch.cuda.device(x.device):
        L.check(L.load().dfft_fft1d_cols(x.data_ptr(), out.data_ptr(), x.shape[1], x.shape[2], x.shape[0], _dtype_code(x),
                                         direction, None), "dfft_fft1d_cols")
        torch.cuda.synchronize()
    return out


def length_kind(n: int) -> int:
    """How length n is computed (dfft_length_kind): 1 single-pass, 2 four-step, 3 Bluestein (fft1d_any, PLAN_ANY_LENGTH), 0 none."""
    return int(L.load().dfft_length_kind(int(n)))


def bluestein_length(n: int) -> int:
    """The padded length M >= 2n - 1 of a Bluestein transform of length n (dfft_bluestein_length); 0 if n is not of kind 3."""
    return int(L.load().dfft_bluestein_length(int(n)))


def fft1d_any(x, dim: int = -1, direction: int = FORWARD, out=None):
    """Length-n FFT along dimension `dim` of a contiguous complex device tensor, for any n up to 2^23 (dfft_fft1d_any): the tensor is
    seen as [batch][n][s] (batch = the dimensions before `dim`, s = those after it).  Kind 1 and 2 lengths give exactly the results of
    fft1d_rows / fft1d_cols; other lengths run Bluestein's algorithm.  Unnormalised; out=x transforms in place."""
    import math

    import torch
    assert x.is_cuda and x.is_contiguous() and x.dim() >= 1
    out = _check_out(x, out)
    d = dim % x.dim()
    n = int(x.shape[d])
    batch = math.prod(int(v) for v in x.shape[:d])
    s = math.prod(int(v) for v in x.shape[d + 1:])
    with torch.cuda.device(x.device):
        L.check(L.load().dfft_fft1d_any(x.data_ptr(), out.data_ptr(), n, s, batch, _dtype_code(x), direction, None), "dfft_fft1d_any")
        torch.cuda.synchronize()
    return out


def real_form(n: int) -> int:
    """How a real transform of length n is computed (dfft_real_form): 1 half-length, 2 paired single-pass, 3 paired four-step /
    Bluestein, 0 none."""
    return int(L.load().dfft_real_form(int(n)))


def _axis_split(shape, dim):
    """(batch, n, s) of a contiguous tensor seen as [batch][n][s] along dimension `dim` (-ndim <= dim < ndim, as in torch and numpy)."""
    import math
    if not -len(shape) <= dim < len(shape):
        raise IndexError(f"dim {dim} is out of range for a tensor of {len(shape)} dimensions")
    d = dim % len(shape)
    return math.prod(int(v) for v in shape[:d]), int(shape[d]), math.prod(int(v) for v in shape[d + 1:]), d


def rfft1d(x, out=None, *, dim: int = -1):
    """numpy.fft.rfft along dimension `dim` of a contiguous float64 / float32 device tensor -> complex128 / complex64 with n//2 + 1 bins
    in that dimension, for any n with real_form(n) != 0: the last dimension through dfft_rfft1d, any other through dfft_rfft1d_strided
    (the tensor seen as [batch][n][s]).  Unnormalised, out of place."""
    import torch
    assert x.is_cuda and x.is_contiguous() and x.dim() >= 1 and x.dtype in (torch.float64, torch.float32)
    batch, n, s, d = _axis_split(x.shape, dim)
    cdt = torch.complex128 if x.dtype == torch.float64 else torch.complex64
    shape = tuple(x.shape[:d]) + (n // 2 + 1,) + tuple(x.shape[d + 1:])
    if out is None:
        out = torch.empty(shape, dtype=cdt, device=x.device)
    assert tuple(out.shape) == shape and out.dtype == cdt and out.device == x.device and out.is_contiguous(), \
        f"out must be a contiguous {cdt} tensor of shape {shape} on {x.device}"
    code = F64 if x.dtype == torch.float64 else F32
    with torch.cuda.device(x.device):
        if s == 1:
            L.check(L.load().dfft_rfft1d(x.data_ptr(), out.data_ptr(), n, batch, code, FORWARD, None), "dfft_rfft1d")
        else:
            L.check(L.load().dfft_rfft1d_strided(x.data_ptr(), out.data_ptr(), n, s, batch, code, FORWARD, None), "dfft_rfft1d_strided")
        torch.cuda.synchronize()
    return out


def irfft1d(X, n: int, out=None, *, dim: int = -1):
    """n * numpy.fft.irfft(X, n, axis=dim) of a contiguous complex128 / complex64 device tensor with n//2 + 1 bins in dimension `dim`
    -> float64 / float32 with n reals there (dfft_rfft1d / dfft_rfft1d_strided, backward): unnormalised; the imaginary parts of bin 0
    and, n even, bin n/2 are ignored.  X is left untouched."""
    import torch
    assert X.is_cuda and X.is_contiguous() and X.dim() >= 1 and X.dtype in (torch.complex128, torch.complex64)
    n = int(n)
    batch, nh, s, d = _axis_split(X.shape, dim)
    assert nh == n // 2 + 1, f"irfft1d: dimension {d} must hold n//2 + 1 = {n // 2 + 1} bins, got {nh}"
    rdt = torch.float64 if X.dtype == torch.complex128 else torch.float32
    shape = tuple(X.shape[:d]) + (n,) + tuple(X.shape[d + 1:])
    if out is None:
        out = torch.empty(shape, dtype=rdt, device=X.device)
    assert tuple(out.shape) == shape and out.dtype == rdt and out.device == X.device and out.is_contiguous(), \
        f"out must be a contiguous {rdt} tensor of shape {shape} on {X.device}"
    code = F64 if rdt == torch.float64 else F32
    with torch.cuda.device(X.device):
        if s == 1:
            L.check(L.load().dfft_rfft1d(X.data_ptr(), out.data_ptr(), n, batch, code, BACKWARD, None), "dfft_rfft1d")
        else:
            L.check(L.load().dfft_rfft1d_strided(X.data_ptr(), out.data_ptr(), n, s, batch, code, BACKWARD, None), "dfft_rfft1d_strided")
        torch.cuda.synchronize()
    return out


R2R_KINDS = {"dct2": L.R2R_DCT2, "dct3": L.R2R_DCT3, "dst2": L.R2R_DST2, "dst3": L.R2R_DST3}


def _r2r_enqueue(src, dst, kind: str, dim: int) -> None:
    if kind not in R2R_KINDS:
        raise ValueError(f"kind must be one of {sorted(R2R_KINDS)}, got {kind!r}")
    import torch
    batch, n, s, _ = _axis_split(src.shape, dim)
    code = F64 if src.dtype == torch.float64 else F32
    L.check(L.load().dfft_r2r1d_strided(src.data_ptr(), dst.data_ptr(), n, s, batch, code, R2R_KINDS[kind], None), "dfft_r2r1d_strided")


def r2r(x, kind: str, dim: int = -1, out=None):
    """DCT / DST of type II or III (kind "dct2" | "dct3" | "dst2" | "dst3") along dimension `dim` of a contiguous float64 / float32
    device tensor (dfft_r2r1d_strided, the tensor seen as [batch][n][s]), for any n with length_kind(n) != 0.  Unnormalised, scipy.fft's
    norm=None: type III of type II is 2n x.  Types I and IV are not built.  out=x transforms in place."""
    import torch
    assert x.is_cuda and x.is_contiguous() and x.dim() >= 1 and x.dtype in (torch.float64, torch.float32) and x.numel() > 0
    out = _check_out(x, out)
    with torch.cuda.device(x.device):
        _r2r_enqueue(x, out, kind, dim)
        torch.cuda.synchronize()
    return out


def r2rn(x, kinds, dims=None, out=None):
    """One r2r per listed dimension, in sequence: kinds[i] along dims[i] (dims=None: the last len(kinds) dimensions), the kinds mixed
    freely -- r2rn(f, ["dct2"] * 3) is the 3-D DCT-II of a single-GPU array.  The first transform goes from x to out, the others run in
    place on out; out=x transforms in place."""
    import torch
    assert x.is_cuda and x.is_contiguous() and x.dim() >= 1 and x.dtype in (torch.float64, torch.float32) and x.numel() > 0
    kinds = list(kinds)
    dims = list(range(x.dim() - len(kinds), x.dim())) if dims is None else [int(d) for d in dims]
    if len(kinds) != len(dims) or not kinds:
        raise ValueError("r2rn: one kind per dimension, at least one")
    for d in dims:
        if not -x.dim() <= d < x.dim():
            raise IndexError(f"dim {d} is out of range for a tensor of {x.dim()} dimensions")
    if len({d % x.dim() for d in dims}) != len(dims):
        raise ValueError("r2rn: a dimension is listed twice")
    for k in kinds:
        if k not in R2R_KINDS:
            raise ValueError(f"kind must be one of {sorted(R2R_KINDS)}, got {k!r}")
    out = _check_out(x, out)
    with torch.cuda.device(x.device):
        src = x
        for k, d in zip(kinds, dims):
            _r2r_enqueue(src, out, k, d)
            src = out
        torch.cuda.synchronize()
    return out


def rconv1d_length(at_least: int) -> int:
    """The smallest padded length m >= at_least that rconv1d accepts (dfft_rconv1d_length: m even, m/2 a single-pass length, so at most
    8192); 0 if there is none."""
    return int(L.load().dfft_rconv1d_length(int(at_least)))


def _rconv1d_args(x, H, m):
    """The argument checks of rconv1d -> (m, channels, n, batch)"""
    import math

    import torch
    assert x.is_cuda and x.is_contiguous() and x.dim() >= 2 and x.dtype in (torch.float64, torch.float32) and x.numel() > 0
    channels, n = int(x.shape[-2]), int(x.shape[-1])
    cdt = torch.complex128 if x.dtype == torch.float64 else torch.complex64
    assert H.is_cuda and H.device == x.device and H.is_contiguous() and H.dim() == 2 and H.dtype in (cdt, x.dtype), \
        f"H must be a contiguous {cdt} or {x.dtype} tensor (channels, m//2 + 1) on {x.device}"
    m = 2 * (int(H.shape[-1]) - 1) if m is None else int(m)
    assert tuple(H.shape) == (channels, m // 2 + 1), f"H must have shape {(channels, m // 2 + 1)}, got {tuple(H.shape)}"
    return m, channels, n, math.prod(int(v) for v in x.shape[:-2])


def _rconv1d_run(x, H, m, out):
    """rconv1d without autograd: one dfft_rconv1d call"""
    import torch
    m, channels, n, batch = _rconv1d_args(x, H, m)
    out = _check_out(x, out)
    with torch.cuda.device(x.device):
        L.check(L.load().dfft_rconv1d(x.data_ptr(), out.data_ptr(), H.data_ptr(), n, m, channels, batch, F64 if x.dtype == torch.float64 else F32,
                                      FILTER_REAL if H.dtype == x.dtype else FILTER_COMPLEX, None), "dfft_rconv1d")
        torch.cuda.synchronize()
    return out


def _fftconv1d_filter(k, m):
    """rfft1d of the taps k (channels, taps) zero-padded to m"""
    import torch
    kp = torch.zeros((int(k.shape[0]), m), dtype=k.dtype, device=k.device)
    kp[:, :int(k.shape[-1])] = k
    return rfft1d(kp)


_AUTOGRAD = []


def _autograd_functions():
    """(rconv1d, fftconv1d) as torch.autograd.Function subclasses, defined on first use: this module imports torch inside functions only.
        grad_x = rconv1d(g, conj(H), m)
        grad_H = w / m * rxspec1d(x, g, m),  w = 1 at bins 0 and m/2, 2 elsewhere (its real part for a real H)
        grad_k = irfft1d(rxspec1d(x, g, m), m)[:, :taps] / m
    (g: the gradient of the output).  Backward is once_differentiable and launches nothing for an input that needs no gradient."""
    if _AUTOGRAD:
        return _AUTOGRAD[0]
    import torch
    from torch.autograd.function import once_differentiable

    def grad_x(g, H, m):
        return _rconv1d_run(g, H.conj().resolve_conj().contiguous() if H.is_complex() else H, m, None)

    class Rconv1dFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, H, m):
            ctx.save_for_backward(x, H)
            ctx.m = m
            return _rconv1d_run(x, H, m, None)

        @staticmethod
        @once_differentiable
        def backward(ctx, g):
            x, H = ctx.saved_tensors
            g = g.contiguous()
            gx = grad_x(g, H, ctx.m) if ctx.needs_input_grad[0] else None
            gH = None
            if ctx.needs_input_grad[1]:
                gH = rxspec1d(x, g, ctx.m)
                w = torch.full((ctx.m // 2 + 1,), 2.0 / ctx.m, dtype=x.dtype, device=x.device)
                w[0] = w[-1] = 1.0 / ctx.m
                gH = gH * w if H.is_complex() else (gH.real * w).contiguous()
            return gx, gH, None

    class Fftconv1dFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, k, m):
            H = _fftconv1d_filter(k, m)
            ctx.save_for_backward(x, H)
            ctx.m, ctx.taps = m, int(k.shape[-1])
            return _rconv1d_run(x, H, m, None)

        @staticmethod
        @once_differentiable
        def backward(ctx, g):
            x, H = ctx.saved_tensors
            g = g.contiguous()
            gx = grad_x(g, H, ctx.m) if ctx.needs_input_grad[0] else None
            gk = None
            if ctx.needs_input_grad[1]:
                gk = (irfft1d(rxspec1d(x, g, ctx.m), ctx.m)[:, :ctx.taps] / ctx.m).contiguous()
            return gx, gk, None

    _AUTOGRAD.append((Rconv1dFn, Fftconv1dFn))
    return _AUTOGRAD[0]


def _wants_grad(*tensors):
    import torch
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


def rxspec1d(x, g, m: int, out=None):
    """S[c, k] = sum over the batch of conj(numpy.fft.rfft(x[..., c, :], m)[k]) * numpy.fft.rfft(g[..., c, :], m)[k], k = 0 ... m//2, for two
    contiguous float64 / float32 device tensors (..., channels, n) of one shape (dfft_rxspec1d) -> (channels, m//2 + 1) of the matching
    complex dtype, unnormalised.  m must be a length rconv1d_length returns.  g is x gives the auto-spectrum sum |X|^2 with exact-zero
    imaginary parts.  The result is the same bits from call to call.  The framed, windowed (Welch) sum is rcsd1d.  Autograd of rxspec1d
    itself is not built."""
    import math

    import torch
    assert x.is_cuda and x.is_contiguous() and x.dim() >= 2 and x.dtype in (torch.float64, torch.float32) and x.numel() > 0
    assert g.is_cuda and g.device == x.device and g.is_contiguous() and g.dtype == x.dtype and g.shape == x.shape, \
        f"g must be a contiguous {x.dtype} tensor of shape {tuple(x.shape)} on {x.device}"
    m = int(m)
    channels, n = int(x.shape[-2]), int(x.shape[-1])
    cdt = torch.complex128 if x.dtype == torch.float64 else torch.complex64
    shape = (channels, m // 2 + 1)
    if out is None:
        out = torch.empty(shape, dtype=cdt, device=x.device)
    assert tuple(out.shape) == shape and out.dtype == cdt and out.device == x.device and out.is_contiguous(), \
        f"out must be a contiguous {cdt} tensor of shape {shape} on {x.device}"
    batch = math.prod(int(v) for v in x.shape[:-2])
    with torch.cuda.device(x.device):
        L.check(L.load().dfft_rxspec1d(x.data_ptr(), g.data_ptr(), out.data_ptr(), n, m, channels, batch, F64 if x.dtype == torch.float64 else F32, None),
                "dfft_rxspec1d")
        torch.cuda.synchronize()
    return out


def rconv1d(x, H, m: Optional[int] = None, out=None):
    """y[..., c, :] = numpy.fft.irfft(numpy.fft.rfft(x[..., c, :], m) * H[c], m)[:n] for every row of a contiguous float64 / float32
    device tensor (..., channels, n) (dfft_rconv1d).  H is (channels, m//2 + 1) of the matching complex dtype, or of x's own dtype (a
    real filter: half the filter bytes); m defaults to 2 * (H.shape[-1] - 1) and must be a length rconv1d_length returns.  m == n is
    the circular convolution, m >= n + taps - 1 the head of the linear one.  Normalised: H == 1 gives y == x.  out=x runs in place.
    Differentiable in x and H (grad mode on and either requires grad; out= is then a ValueError): the input gradient is rconv1d with the
    conjugated filter, the filter gradient rxspec1d.  Double backward is not built, and rconv1d_os / fftfilt1d are not differentiable
    (rconv1d_long / fftconv1d_long are)."""
    if _wants_grad(x, H):
        if out is not None:
            raise ValueError("rconv1d: out= cannot be combined with a tensor that requires grad")
        m = _rconv1d_args(x, H, m)[0]
        return _autograd_functions()[0].apply(x, H, m)
    return _rconv1d_run(x, H, m, out)


def fftconv1d(x, k, out=None):
    """numpy.convolve(x[..., c, :], k[c])[:n] for every row of a contiguous float64 / float32 device tensor (..., channels, n): the
    causal "long convolution" with the real taps k (channels, taps), through rconv1d on m = rconv1d_length(n + taps - 1) with the
    filter spectrum rfft1d of the zero-padded taps.  n + taps - 1 must not exceed 8192.  Differentiable in x and k (grad mode on and
    either requires grad; out= is then a ValueError); double backward is not built."""
    assert x.is_cuda and x.dim() >= 2 and k.is_cuda and k.dim() == 2 and k.dtype == x.dtype and k.device == x.device
    channels, n, taps = int(x.shape[-2]), int(x.shape[-1]), int(k.shape[-1])
    assert int(k.shape[0]) == channels, f"k must hold one row of taps per channel: ({channels}, taps), got {tuple(k.shape)}"
    m = rconv1d_length(n + taps - 1)
    if m == 0:
        raise ValueError(f"fftconv1d: n + taps - 1 = {n + taps - 1} is beyond the longest padded length (8192)")
    if _wants_grad(x, k):
        if out is not None:
            raise ValueError("fftconv1d: out= cannot be combined with a tensor that requires grad")
        assert x.is_contiguous() and x.dtype.is_floating_point and x.numel() > 0
        return _autograd_functions()[1].apply(x, k, m)
    return rconv1d(x, _fftconv1d_filter(k, m), m, out=out)


def rconv1d_long_length(at_least: int) -> int:
    """The smallest padded length m >= at_least that rconv1d_long accepts (dfft_rconv1d_long_length: m even, 8192 < m <= 2^23, m/2 a
    product of two tuned single-pass lengths); 0 if there is none."""
    return int(L.load().dfft_rconv1d_long_length(int(at_least)))


def rconv1d_long_filter(H, m: Optional[int] = None):
    """The filter H (channels, m//2 + 1) of rconv1d, complex or real, in the order rconv1d_long reads it (dfft_rconv1d_long_filter): a
    new tensor of the same shape and dtype, Hp[c, k1 * N2 + k2] = H[c, k1 + N1 * k2], Hp[c, m//2] = H[c, m//2] for the split
    m//2 = N1 * N2 of the library.  m defaults to 2 * (H.shape[-1] - 1)."""
    import torch
    assert H.is_cuda and H.is_contiguous() and H.dim() == 2 and H.dtype in (torch.complex128, torch.complex64, torch.float64, torch.float32), \
        "H must be a contiguous complex or real device tensor (channels, m//2 + 1)"
    m = 2 * (int(H.shape[-1]) - 1) if m is None else int(m)
    assert int(H.shape[-1]) == m // 2 + 1, f"H must have shape (channels, {m // 2 + 1}), got {tuple(H.shape)}"
    Hp = torch.empty_like(H)
    with torch.cuda.device(H.device):
        L.check(L.load().dfft_rconv1d_long_filter(H.data_ptr(), Hp.data_ptr(), m, int(H.shape[0]),
                                                  F64 if H.dtype in (torch.complex128, torch.float64) else F32,
                                                  FILTER_COMPLEX if H.dtype.is_complex else FILTER_REAL, None), "dfft_rconv1d_long_filter")
        torch.cuda.synchronize()
    return Hp


def _rconv1d_long_args(x, Hp, m):
    """The argument checks of rconv1d_long -> (m, channels, n, batch)"""
    import math

    import torch
    assert x.is_cuda and x.is_contiguous() and x.dim() >= 2 and x.dtype in (torch.float64, torch.float32) and x.numel() > 0
    channels, n = int(x.shape[-2]), int(x.shape[-1])
    cdt = torch.complex128 if x.dtype == torch.float64 else torch.complex64
    assert Hp.is_cuda and Hp.device == x.device and Hp.is_contiguous() and Hp.dim() == 2 and Hp.dtype in (cdt, x.dtype), \
        f"Hp must be a contiguous {cdt} or {x.dtype} tensor (channels, m//2 + 1) on {x.device}"
    m = 2 * (int(Hp.shape[-1]) - 1) if m is None else int(m)
    assert tuple(Hp.shape) == (channels, m // 2 + 1), f"Hp must have shape {(channels, m // 2 + 1)}, got {tuple(Hp.shape)}"
    return m, channels, n, math.prod(int(v) for v in x.shape[:-2])


def _rconv1d_long_run(x, Hp, m, out):
    """rconv1d_long without autograd: one dfft_rconv1d_long call"""
    import torch
    m, channels, n, batch = _rconv1d_long_args(x, Hp, m)
    cdt = torch.complex128 if x.dtype == torch.float64 else torch.complex64
    out = _check_out(x, out)
    with torch.cuda.device(x.device):
        L.check(L.load().dfft_rconv1d_long(x.data_ptr(), out.data_ptr(), Hp.data_ptr(), n, m, channels, batch,
                                           F64 if x.dtype == torch.float64 else F32, FILTER_COMPLEX if Hp.dtype == cdt else FILTER_REAL, None),
                "dfft_rconv1d_long")
        torch.cuda.synchronize()
    return out


def _fftconv1d_long_filter(k, m):
    """rfft1d of the taps k (channels, taps) zero-padded to m, in the order rconv1d_long reads it"""
    import torch
    kp = torch.zeros((int(k.shape[0]), m), dtype=k.dtype, device=k.device)
    kp[:, :int(k.shape[-1])] = k
    return rconv1d_long_filter(rfft1d(kp))


_AUTOGRAD_LONG = []


def _autograd_functions_long():
    """(rconv1d_long, fftconv1d_long) as torch.autograd.Function subclasses, defined on first use (see _autograd_functions):
        grad_x  = rconv1d_long(g, conj(Hp), m)          (conjugation commutes with the permutation of rconv1d_long_filter)
        grad_Hp = w / m * rxspec1d_long(x, g, m, filter_order=True),  w = 1 at bins 0 and m/2 -- positions 0 and m/2 of the permuted
                  order as well -- and 2 elsewhere (its real part for a real Hp)
        grad_k  = irfft1d(rxspec1d_long(x, g, m), m)[:, :taps] / m
    (g: the gradient of the output).  Backward is once_differentiable and launches nothing for an input that needs no gradient."""
    if _AUTOGRAD_LONG:
        return _AUTOGRAD_LONG[0]
    import torch
    from torch.autograd.function import once_differentiable

    def grad_x(g, Hp, m):
        return _rconv1d_long_run(g, Hp.conj().resolve_conj().contiguous() if Hp.is_complex() else Hp, m, None)

    class Rconv1dLongFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, Hp, m):
            ctx.save_for_backward(x, Hp)
            ctx.m = m
            return _rconv1d_long_run(x, Hp, m, None)

        @staticmethod
        @once_differentiable
        def backward(ctx, g):
            x, Hp = ctx.saved_tensors
            g = g.contiguous()
            gx = grad_x(g, Hp, ctx.m) if ctx.needs_input_grad[0] else None
            gH = None
            if ctx.needs_input_grad[1]:
                gH = rxspec1d_long(x, g, ctx.m, filter_order=True)
                w = torch.full((ctx.m // 2 + 1,), 2.0 / ctx.m, dtype=x.dtype, device=x.device)
                w[0] = w[-1] = 1.0 / ctx.m
                gH = gH * w if Hp.is_complex() else (gH.real * w).contiguous()
            return gx, gH, None

    class Fftconv1dLongFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, k, m):
            Hp = _fftconv1d_long_filter(k, m)
            ctx.save_for_backward(x, Hp)
            ctx.m, ctx.taps = m, int(k.shape[-1])
            return _rconv1d_long_run(x, Hp, m, None)

        @staticmethod
        @once_differentiable
        def backward(ctx, g):
            x, Hp = ctx.saved_tensors
            g = g.contiguous()
            gx = grad_x(g, Hp, ctx.m) if ctx.needs_input_grad[0] else None
            gk = None
            if ctx.needs_input_grad[1]:
                gk = (irfft1d(rxspec1d_long(x, g, ctx.m), ctx.m)[:, :ctx.taps] / ctx.m).contiguous()
            return gx, gk, None

    _AUTOGRAD_LONG.append((Rconv1dLongFn, Fftconv1dLongFn))
    return _AUTOGRAD_LONG[0]


def rxspec1d_long(x, g, m: int, out=None, filter_order: bool = False):
    """rxspec1d for padded lengths beyond 8192 (dfft_rxspec1d_long): S[c, k] = sum over the batch of conj(numpy.fft.rfft(x[..., c, :], m)[k])
    * numpy.fft.rfft(g[..., c, :], m)[k], k = 0 ... m//2, for two contiguous float64 / float32 device tensors (..., channels, n) of one
    shape -> (channels, m//2 + 1) of the matching complex dtype, unnormalised.  m must be a length rconv1d_long_length returns.
    filter_order=True returns the layout of rconv1d_long_filter (S[c, k1 + N1 * k2] at position k1 * N2 + k2).  g is x gives the
    auto-spectrum sum |X|^2 with exact-zero imaginary parts.  The result is the same bits from call to call.  The framed,
    windowed (Welch) sum is rcsd1d, for frames of at most 8192 samples.  Autograd of rxspec1d_long itself is not built."""
    import math

    import torch
    assert x.is_cuda and x.is_contiguous() and x.dim() >= 2 and x.dtype in (torch.float64, torch.float32) and x.numel() > 0
    assert g.is_cuda and g.device == x.device and g.is_contiguous() and g.dtype == x.dtype and g.shape == x.shape, \
        f"g must be a contiguous {x.dtype} tensor of shape {tuple(x.shape)} on {x.device}"
    m = int(m)
    channels, n = int(x.shape[-2]), int(x.shape[-1])
    cdt = torch.complex128 if x.dtype == torch.float64 else torch.complex64
    shape = (channels, m // 2 + 1)
    if out is None:
        out = torch.empty(shape, dtype=cdt, device=x.device)
    assert tuple(out.shape) == shape and out.dtype == cdt and out.device == x.device and out.is_contiguous(), \
        f"out must be a contiguous {cdt} tensor of shape {shape} on {x.device}"
    batch = math.prod(int(v) for v in x.shape[:-2])
    with torch.cuda.device(x.device):
        L.check(L.load().dfft_rxspec1d_long(x.data_ptr(), g.data_ptr(), out.data_ptr(), n, m, channels, batch,
                                            F64 if x.dtype == torch.float64 else F32, 1 if filter_order else 0, None), "dfft_rxspec1d_long")
        torch.cuda.synchronize()
    return out


def rconv1d_long(x, Hp, m: Optional[int] = None, out=None):
    """rconv1d for padded lengths beyond 8192 (dfft_rconv1d_long): y[..., c, :] = numpy.fft.irfft(numpy.fft.rfft(x[..., c, :], m) * H[c],
    m)[:n] for every row of a contiguous float64 / float32 device tensor (..., channels, n), with Hp = rconv1d_long_filter(H).  m
    defaults to 2 * (Hp.shape[-1] - 1) and must be a length rconv1d_long_length returns.  Normalised: H == 1 gives y == x.  out=x runs
    in place.  Differentiable in x and Hp, complex or real (grad mode on and either requires grad; out= is then a ValueError): the
    input gradient is rconv1d_long with the conjugated filter, the filter gradient rxspec1d_long in the filter's order.  Double
    backward is not built."""
    if _wants_grad(x, Hp):
        if out is not None:
            raise ValueError("rconv1d_long: out= cannot be combined with a tensor that requires grad")
        m = _rconv1d_long_args(x, Hp, m)[0]
        return _autograd_functions_long()[0].apply(x, Hp, m)
    return _rconv1d_long_run(x, Hp, m, out)


def fftconv1d_long(x, k, out=None):
    """fftconv1d for n + taps - 1 > 8192: numpy.convolve(x[..., c, :], k[c])[:n] for every row of a contiguous float64 / float32 device
    tensor (..., channels, n) with the real taps k (channels, taps), through rconv1d_long on m = rconv1d_long_length(n + taps - 1) with
    the filter spectrum rfft1d of the zero-padded taps.  n + taps - 1 must not exceed 2^23.  Differentiable in x and k (grad mode on
    and either requires grad; out= is then a ValueError); double backward is not built."""
    assert x.is_cuda and x.dim() >= 2 and k.is_cuda and k.dim() == 2 and k.dtype == x.dtype and k.device == x.device
    channels, n, taps = int(x.shape[-2]), int(x.shape[-1]), int(k.shape[-1])
    assert int(k.shape[0]) == channels, f"k must hold one row of taps per channel: ({channels}, taps), got {tuple(k.shape)}"
    if n + taps - 1 <= 8192:
        raise ValueError(f"fftconv1d_long: n + taps - 1 = {n + taps - 1} is within the single-pass range (at most 8192): use fftconv1d")
    m = rconv1d_long_length(n + taps - 1)
    if m == 0:
        raise ValueError(f"fftconv1d_long: n + taps - 1 = {n + taps - 1} is beyond the longest padded length (2^23)")
    if _wants_grad(x, k):
        if out is not None:
            raise ValueError("fftconv1d_long: out= cannot be combined with a tensor that requires grad")
        assert x.is_contiguous() and x.dtype.is_floating_point and x.numel() > 0
        return _autograd_functions_long()[1].apply(x, k, m)
    return rconv1d_long(x, _fftconv1d_long_filter(k, m), m, out=out)


def rconv1d_os_block(taps: int, n_out: int, dtype) -> tuple:
    """(m, discard) that dfft_rconv1d_os_block chooses for `taps` taps and n_out results per row of a float64 / float32 tensor (dtype a
    torch dtype or F64 / F32): discard = taps - 1 rounded up to even, m the accepted block length with the smallest estimated time.
    ValueError beyond 8191 taps."""
    import ctypes as C
    if not isinstance(dtype, int):
        import torch
        assert dtype in (torch.float64, torch.float32)
        dtype = F64 if dtype == torch.float64 else F32
    m, d = C.c_longlong(0), C.c_longlong(0)
    rc = L.load().dfft_rconv1d_os_block(int(taps), int(n_out), int(dtype), C.byref(m), C.byref(d))
    if rc == L.EUNSUPPORTED:
        raise ValueError(f"rconv1d_os_block: {taps} taps are beyond the longest block (8191 taps)")
    L.check(rc, "dfft_rconv1d_os_block")
    return int(m.value), int(d.value)


def rconv1d_os(x, H, m: Optional[int] = None, discard: int = 0, n_out: Optional[int] = None, out=None):
    """Overlap-save rconv1d for rows of any length (dfft_rconv1d_os): x (..., channels, n) -> (..., channels, n_out), in blocks of m reals
    that advance by S = m - discard; block b of a row is irfft(rfft(x[b S - discard : b S - discard + m], m) * H[c], m) with zeros outside
    the row, and its results from `discard` on become y[b S : b S + S].  H as in rconv1d, m defaults to 2 * (H.shape[-1] - 1), n_out to
    n (at most n + discard).  With H the spectrum of taps <= discard + 1 taps this is numpy.convolve(x, k)[:n_out].  Out of place only."""
    import math

    import torch
    assert x.is_cuda and x.is_contiguous() and x.dim() >= 2 and x.dtype in (torch.float64, torch.float32) and x.numel() > 0
    channels, n = int(x.shape[-2]), int(x.shape[-1])
    cdt = torch.complex128 if x.dtype == torch.float64 else torch.complex64
    assert H.is_cuda and H.device == x.device and H.is_contiguous() and H.dim() == 2 and H.dtype in (cdt, x.dtype), \
        f"H must be a contiguous {cdt} or {x.dtype} tensor (channels, m//2 + 1) on {x.device}"
    m = 2 * (int(H.shape[-1]) - 1) if m is None else int(m)
    assert tuple(H.shape) == (channels, m // 2 + 1), f"H must have shape {(channels, m // 2 + 1)}, got {tuple(H.shape)}"
    n_out = n if n_out is None else int(n_out)
    shape = tuple(x.shape[:-1]) + (n_out,)
    if out is None:
        out = torch.empty(shape, dtype=x.dtype, device=x.device)
    assert out.is_cuda and out.device == x.device and out.is_contiguous() and out.dtype == x.dtype and tuple(out.shape) == shape, \
        f"out must be a contiguous {x.dtype} tensor of shape {shape} on {x.device}"
    batch = math.prod(int(v) for v in x.shape[:-2])
    with torch.cuda.device(x.device):
        L.check(L.load().dfft_rconv1d_os(x.data_ptr(), out.data_ptr(), H.data_ptr(), n, n_out, m, int(discard), channels, batch,
                                         F64 if x.dtype == torch.float64 else F32, FILTER_COMPLEX if H.dtype == cdt else FILTER_REAL, None), "dfft_rconv1d_os")
        torch.cuda.synchronize()
    return out


def fftfilt1d(x, k, mode: str = "head", m: Optional[int] = None, out=None):
    """numpy.convolve(x[..., c, :], k[c]) for every row of a contiguous float64 / float32 device tensor (..., channels, n) of ANY length
    with the real taps k (channels, taps), taps <= 8191: its first n samples (mode "head", the causal filter) or all n + taps - 1
    (mode "full").  Overlap-save through rconv1d_os: the block (m, discard) comes from rconv1d_os_block unless m is given (then discard
    = taps - 1 rounded up to even, which m must exceed); the filter spectrum is rfft1d of the taps zero-padded to m."""
    import torch
    assert x.is_cuda and x.dim() >= 2 and k.is_cuda and k.dim() == 2 and k.dtype == x.dtype and k.device == x.device
    if mode not in ("head", "full"):
        raise ValueError(f"mode must be 'head' or 'full', got {mode!r}")
    channels, n, taps = int(x.shape[-2]), int(x.shape[-1]), int(k.shape[-1])
    assert int(k.shape[0]) == channels, f"k must hold one row of taps per channel: ({channels}, taps), got {tuple(k.shape)}"
    n_out = n if mode == "head" else n + taps - 1
    if m is None:
        m, discard = rconv1d_os_block(taps, n_out, x.dtype)
    else:
        m, discard = int(m), taps - 1 + ((taps - 1) & 1)
        if m <= discard:
            raise ValueError(f"fftfilt1d: a block of m = {m} leaves no room behind the {discard} samples that {taps} taps discard")
    kp = torch.zeros((channels, m), dtype=k.dtype, device=k.device)
    kp[:, :taps] = k
    return rconv1d_os(x, rfft1d(kp), m, discard, n_out, out=out)


STFT_PAD_ZERO, STFT_PAD_REFLECT = 0, 1
STFT_OUT_COMPLEX, STFT_OUT_POWER = 0, 1


def stft_frames(n: int, n_fft: int, hop: int, pad: int) -> int:
    """Frames that rows of n samples give (dfft_stft1d_frames): 1 + (n + 2 pad - n_fft) // hop where n + 2 pad >= n_fft, else 0."""
    return int(L.load().dfft_stft1d_frames(int(n), int(n_fft), int(hop), int(pad)))


def _stft_window(window, n_fft, win_length, dtype, device):
    """The window of n_fft reals the library takes: ones (window None), or `window` of win_length values centred and zero-padded."""
    import torch
    win_length = n_fft if win_length is None else int(win_length)
    if not 1 <= win_length <= n_fft:
        raise ValueError(f"win_length must be in [1, n_fft = {n_fft}], got {win_length}")
    if window is None:
        w = torch.ones(win_length, dtype=dtype, device=device)
    else:
        if window.dim() != 1 or int(window.shape[0]) != win_length:
            raise ValueError(f"window must be a 1-D tensor of win_length = {win_length} values, got shape {tuple(window.shape)}")
        w = window.to(device=device, dtype=dtype)
    if win_length < n_fft:
        left = (n_fft - win_length) // 2
        w = torch.nn.functional.pad(w, (left, n_fft - win_length - left))
    return w.contiguous()


def stft(x, n_fft: int, hop_length: Optional[int] = None, window=None, center: bool = True, pad_mode: str = "reflect", normalized: bool = False,
         win_length: Optional[int] = None, frames_last: bool = True, power=None, out=None):
    """torch.stft(x, n_fft, hop_length, win_length, window, center, pad_mode, normalized, onesided=True, return_complex=True) of a
    contiguous float64 / float32 device tensor (..., n) (dfft_stft1d): frames of n_fft samples that advance by hop_length (default
    n_fft // 4), each multiplied by the window (None: rectangular; win_length < n_fft: centred and zero-padded) and transformed.
    center pads n_fft // 2 samples on both sides, mirrored (pad_mode "reflect", which needs n_fft // 2 < n) or zero ("constant").
    The storage is (..., frames, bins) contiguous, bins = n_fft // 2 + 1; frames_last=True returns its (..., bins, frames) transposed view
    (torch's order), False the storage itself.  power=2 returns the real power spectrogram |X|^2 (half the bytes) instead of X.
    n_fft must be of real form 1 (even, n_fft // 2 a single-pass length, at most 8192).  `out`: the (..., frames, bins) storage.  No
    autograd."""
    import math

    import torch
    assert x.is_cuda and x.is_contiguous() and x.dim() >= 1 and x.dtype in (torch.float64, torch.float32) and x.numel() > 0
    if pad_mode not in ("reflect", "constant"):
        raise ValueError(f"pad_mode must be 'reflect' or 'constant', got {pad_mode!r}")
    if power not in (None, 2, 2.0):
        raise ValueError(f"power must be None (complex bins) or 2 (the power spectrogram), got {power!r}")
    n_fft, n = int(n_fft), int(x.shape[-1])
    hop = n_fft // 4 if hop_length is None else int(hop_length)
    if hop < 1:
        raise ValueError(f"hop_length must be at least 1, got {hop}")
    pad = n_fft // 2 if center else 0
    if center and pad_mode == "reflect" and pad >= n:
        raise ValueError(f"reflect padding of {pad} samples needs rows longer than that, got n = {n}")
    frames = stft_frames(n, n_fft, hop, pad)
    if frames < 1:
        raise ValueError(f"rows of {n} samples{' (padded)' if center else ''} are shorter than one frame of n_fft = {n_fft}")
    w = _stft_window(window, n_fft, win_length, x.dtype, x.device)
    cdt = torch.complex128 if x.dtype == torch.float64 else torch.complex64
    odt = x.dtype if power is not None else cdt
    shape = tuple(x.shape[:-1]) + (frames, n_fft // 2 + 1)
    if out is None:
        out = torch.empty(shape, dtype=odt, device=x.device)
    assert out.is_cuda and out.device == x.device and out.is_contiguous() and out.dtype == odt and tuple(out.shape) == shape, \
        f"out must be a contiguous {odt} tensor of shape {shape} on {x.device}"
    rows = math.prod(int(v) for v in x.shape[:-1])
    with torch.cuda.device(x.device):
        L.check(L.load().dfft_stft1d(x.data_ptr(), out.data_ptr(), w.data_ptr(), n, n_fft, hop, pad, frames, rows, F64 if x.dtype == torch.float64 else F32,
                                     STFT_PAD_REFLECT if (center and pad_mode == "reflect") else STFT_PAD_ZERO,
                                     STFT_OUT_POWER if power is not None else STFT_OUT_COMPLEX, n_fft ** -0.5 if normalized else 1.0, None), "dfft_stft1d")
        torch.cuda.synchronize()
    return out.transpose(-1, -2) if frames_last else out


def istft_envelope(window, n_fft: int, hop: int, frames: int):
    """sum_f win^2[s - f hop] for s in [0, (frames - 1) hop + n_fft): the overlap-add of the squared window, in float64 on its device."""
    import torch
    shifts = -(-n_fft // hop)                                      # frames that reach one sample, at most
    w2 = torch.nn.functional.pad(window.to(torch.float64) ** 2, (0, shifts * hop - n_fft))
    env = torch.zeros((frames - 1 + shifts) * hop, dtype=torch.float64, device=window.device)
    for j in range(shifts):                                        # hop values of win^2 at a time, laid end to end once per frame: O(n) each
        env[j * hop:(j + frames) * hop] += w2[j * hop:(j + 1) * hop].repeat(frames)
    return env[:(frames - 1) * hop + n_fft]


def istft(X, n_fft: int, hop_length: Optional[int] = None, window=None, center: bool = True, normalized: bool = False, win_length: Optional[int] = None,
          length: Optional[int] = None, frames_last: bool = True, out=None):
    """torch.istft(X, n_fft, hop_length, win_length, window, center, normalized, onesided=True, length) of a complex128 / complex64
    device tensor (..., bins, frames) (frames_last=True, torch's order) or (..., frames, bins) (False), bins = n_fft // 2 + 1
    (dfft_istft1d): the least-squares overlap-add sum_f win irfft(X_f) / sum_f win^2.  center drops the n_fft // 2 padded samples in
    front; the result holds `length` samples (default: (frames - 1) hop, or + n_fft without center; beyond the last frame: zeros).
    ValueError where the window envelope sum_f win^2 falls to 1e-11 or below inside the result (torch's NOLA check).  A (..., bins, frames)
    tensor that is not the transposed view of contiguous (..., frames, bins) storage is copied into that layout.  No autograd."""
    import math

    import torch
    assert X.is_cuda and X.dim() >= 2 and X.dtype in (torch.complex128, torch.complex64) and X.numel() > 0
    Xs = X.transpose(-1, -2) if frames_last else X
    if not Xs.is_contiguous():
        Xs = Xs.contiguous()
    n_fft = int(n_fft)
    frames, bins = int(Xs.shape[-2]), int(Xs.shape[-1])
    if bins != n_fft // 2 + 1:
        raise ValueError(f"X must hold n_fft // 2 + 1 = {n_fft // 2 + 1} bins, got {bins}")
    hop = n_fft // 4 if hop_length is None else int(hop_length)
    if hop < 1:
        raise ValueError(f"hop_length must be at least 1, got {hop}")
    rdt = torch.float64 if X.dtype == torch.complex128 else torch.float32
    w = _stft_window(window, n_fft, win_length, rdt, X.device)
    pad = n_fft // 2 if center else 0
    most = (frames - 1) * hop + n_fft - pad                       # samples the frames reach behind the padding in front
    n = (most - pad if center else most) if length is None else int(length)
    if n < 1:
        raise ValueError(f"the result would hold {n} samples")
    have = min(n, most)
    env = istft_envelope(w, n_fft, hop, frames)[pad:pad + have]
    if float(env.abs().min()) <= 1e-11:
        raise ValueError("istft: the window overlap-add envelope falls to 1e-11 or below (NOLA): these frames do not determine the signal")
    inv_env = ((n_fft ** 0.5 if normalized else 1.0) / env).to(rdt).contiguous()
    shape = tuple(Xs.shape[:-2]) + (n,)
    if out is None:
        out = torch.empty(shape, dtype=rdt, device=X.device)
    assert out.is_cuda and out.device == X.device and out.is_contiguous() and out.dtype == rdt and tuple(out.shape) == shape, \
        f"out must be a contiguous {rdt} tensor of shape {shape} on {X.device}"
    rows = math.prod(int(v) for v in Xs.shape[:-2])
    dst = out if have == n else torch.empty(tuple(Xs.shape[:-2]) + (have,), dtype=rdt, device=X.device)
    with torch.cuda.device(X.device):
        L.check(L.load().dfft_istft1d(Xs.data_ptr(), dst.data_ptr(), w.data_ptr(), inv_env.data_ptr(), have, n_fft, hop, pad, frames, rows,
                                      F64 if rdt == torch.float64 else F32, None), "dfft_istft1d")
        torch.cuda.synchronize()
    if dst is not out:
        out[..., :have] = dst
        out[..., have:] = 0
    return out


def rcsd1d(x, g, n_fft: int, hop_length: int, window=None, scale: float = 1.0, out=None, win_length: Optional[int] = None):
    """scale * sum over the frames f of conj(numpy.fft.rfft(w * x[..., f hop : f hop + n_fft])) * numpy.fft.rfft(w * g[..., f hop : f hop + n_fft])
    for two contiguous float64 / float32 device tensors (..., n) of one shape (dfft_rcsd1d) -> (..., n_fft // 2 + 1) of the matching
    complex dtype: the raw sum that welch / csd / coherence average.  Frames are whole and start at sample 0 (no padding, no centring):
    1 + (n - n_fft) // hop_length of them, and the samples behind the last one are not read.  `window`: None (rectangular) or a 1-D
    tensor of win_length (default n_fft) values, centred and zero-padded as in stft.  n_fft must be of real form 1 (even, n_fft // 2 a
    single-pass length, at most 8192).  g is x gives the auto-spectrum with exact-zero imaginary parts.  The result is the same bits
    from call to call.  No autograd."""
    import math

    import torch
    assert x.is_cuda and x.is_contiguous() and x.dim() >= 1 and x.dtype in (torch.float64, torch.float32) and x.numel() > 0
    assert g.is_cuda and g.device == x.device and g.is_contiguous() and g.dtype == x.dtype and g.shape == x.shape, \
        f"g must be a contiguous {x.dtype} tensor of shape {tuple(x.shape)} on {x.device}"
    n_fft, hop, n = int(n_fft), int(hop_length), int(x.shape[-1])
    if hop < 1:
        raise ValueError(f"hop_length must be at least 1, got {hop}")
    frames = stft_frames(n, n_fft, hop, 0)
    if frames < 1:
        raise ValueError(f"rows of {n} samples are shorter than one frame of n_fft = {n_fft}")
    w = _stft_window(window, n_fft, win_length, x.dtype, x.device)
    cdt = torch.complex128 if x.dtype == torch.float64 else torch.complex64
    shape = tuple(x.shape[:-1]) + (n_fft // 2 + 1,)
    if out is None:
        out = torch.empty(shape, dtype=cdt, device=x.device)
    assert out.is_cuda and out.device == x.device and out.is_contiguous() and out.dtype == cdt and tuple(out.shape) == shape, \
        f"out must be a contiguous {cdt} tensor of shape {shape} on {x.device}"
    rows = math.prod(int(v) for v in x.shape[:-1])
    with torch.cuda.device(x.device):
        L.check(L.load().dfft_rcsd1d(x.data_ptr(), g.data_ptr(), out.data_ptr(), w.data_ptr(), n, n_fft, hop, frames, rows, float(scale),
                                     F64 if x.dtype == torch.float64 else F32, None), "dfft_rcsd1d")
        torch.cuda.synchronize()
    return out


def _csd_setup(x, n_fft, hop_length, window, fs, scaling, win_length):
    """hop, window tensor (win_length values) and the scale 1 / (fs sum w^2) ("density") or 1 / (sum w)^2 ("spectrum"), over frames"""
    import torch
    if scaling not in ("density", "spectrum"):
        raise ValueError(f"scaling must be 'density' or 'spectrum', got {scaling!r}")
    n_fft = int(n_fft)
    hop = n_fft // 2 if hop_length is None else int(hop_length)
    wl = n_fft if win_length is None else int(win_length)
    if window is None:
        window = torch.hann_window(wl, periodic=True, dtype=torch.float64, device=x.device)
    w64 = window.to(device=x.device, dtype=x.dtype).to(torch.float64)   # the values the frames are multiplied by
    norm = 1.0 / (float(fs) * float((w64 * w64).sum())) if scaling == "density" else 1.0 / float(w64.sum()) ** 2
    return hop, window, norm


def _one_sided(P, n_fft, norm, frames):
    """the mean over frames, the normalisation, and every bin but 0 and n_fft / 2 doubled -- on the small result"""
    P = P * (norm / frames)
    P[..., 1:n_fft // 2] *= 2.0
    return P


def csd(x, y, n_fft: int, hop_length: Optional[int] = None, window=None, fs: float = 1.0, scaling: str = "density", win_length: Optional[int] = None):
    """scipy.signal.csd(x, y, fs, window, nperseg=n_fft, noverlap=n_fft - hop_length, detrend=False, scaling=scaling) of two contiguous
    float64 / float32 device tensors (..., n) of one shape: the one-sided cross-spectral density (or spectrum) mean_f conj(X_f) Y_f ->
    (..., n_fft // 2 + 1) complex, from one launch of rcsd1d that reads each row once and writes no spectrogram.  hop_length defaults
    to n_fft // 2, window to the periodic Hann window (a 1-D tensor of win_length values otherwise, centred and zero-padded to n_fft).
    Normalisation 1 / (fs sum w^2) for "density", 1 / (sum w)^2 for "spectrum"; every bin but 0 and n_fft / 2 is doubled.
    Not built: per-segment detrending, average="median", two-sided output, padding / boundary extension, frames longer than 8192, and
    autograd."""
    n_fft = int(n_fft)
    hop, window, norm = _csd_setup(x, n_fft, hop_length, window, fs, scaling, win_length)
    P = rcsd1d(x, y, n_fft, hop, window, win_length=win_length)
    return _one_sided(P, n_fft, norm, stft_frames(int(x.shape[-1]), n_fft, hop, 0))


def welch(x, n_fft: int, hop_length: Optional[int] = None, window=None, fs: float = 1.0, scaling: str = "density", win_length: Optional[int] = None):
    """scipy.signal.welch(x, fs, window, nperseg=n_fft, noverlap=n_fft - hop_length, detrend=False, scaling=scaling): the one-sided power
    spectral density (or spectrum) mean_f |X_f|^2 of a contiguous float64 / float32 device tensor (..., n) -> (..., n_fft // 2 + 1) real
    (csd with y is x: the second transform is skipped).  Arguments, and what is not built, as in csd.  No autograd."""
    n_fft = int(n_fft)
    hop, window, norm = _csd_setup(x, n_fft, hop_length, window, fs, scaling, win_length)
    P = rcsd1d(x, x, n_fft, hop, window, win_length=win_length)
    return _one_sided(P.real.contiguous(), n_fft, norm, stft_frames(int(x.shape[-1]), n_fft, hop, 0))


def coherence(x, y, n_fft: int, hop_length: Optional[int] = None, window=None, win_length: Optional[int] = None):
    """scipy.signal.coherence(x, y, window=window, nperseg=n_fft, noverlap=n_fft - hop_length, detrend=False): the magnitude-squared
    coherence |Pxy|^2 / (Pxx Pyy) of two contiguous float64 / float32 device tensors (..., n) of one shape -> (..., n_fft // 2 + 1) real,
    from three launches of rcsd1d (the normalisation cancels).  One frame gives 1.  Arguments, and what is not built, as in csd.  No
    autograd."""
    n_fft = int(n_fft)
    hop, window, _ = _csd_setup(x, n_fft, hop_length, window, 1.0, "density", win_length)
    pxy = rcsd1d(x, y, n_fft, hop, window, win_length=win_length)
    pxx = rcsd1d(x, x, n_fft, hop, window, win_length=win_length).real
    pyy = rcsd1d(y, y, n_fft, hop, window, win_length=win_length).real
    return (pxy.real * pxy.real + pxy.imag * pxy.imag) / (pxx * pyy)


def rfft2d_batch(x, out=None):
    """numpy.fft.rfft2 of every (n1, n2) plane of a contiguous float64 / float32 device tensor [..., n1, n2] -> complex128 / complex64
    [..., n1, n2//2 + 1] (dfft_rfft2d_batch): n2 of any real form, n1 of any length kind.  Unnormalised, out of place."""
    import math

    import torch
    assert x.is_cuda and x.is_contiguous() and x.dim() >= 2 and x.dtype in (torch.float64, torch.float32)
    n1, n2 = int(x.shape[-2]), int(x.shape[-1])
    cdt = torch.complex128 if x.dtype == torch.float64 else torch.complex64
    shape = tuple(x.shape[:-1]) + (n2 // 2 + 1,)
    if out is None:
        out = torch.empty(shape, dtype=cdt, device=x.device)
    assert tuple(out.shape) == shape and out.dtype == cdt and out.device == x.device and out.is_contiguous(), \
        f"out must be a contiguous {cdt} tensor of shape {shape} on {x.device}"
    batch = math.prod(int(v) for v in x.shape[:-2])
    with torch.cuda.device(x.device):
        L.check(L.load().dfft_rfft2d_batch(x.data_ptr(), out.data_ptr(), n1, n2, batch, F64 if x.dtype == torch.float64 else F32, FORWARD,
                                           None), "dfft_rfft2d_batch")
        torch.cuda.synchronize()
    return out


def irfft2d_batch(X, n2: int, out=None):
    """n1 * n2 * numpy.fft.irfft2(X, s=(n1, n2)) of every plane of a contiguous complex128 / complex64 device tensor [..., n1, n2//2 + 1]
    -> float64 / float32 [..., n1, n2] (dfft_rfft2d_batch, backward), for any input.  Unnormalised; X is left untouched."""
    import math

    import torch
    assert X.is_cuda and X.is_contiguous() and X.dim() >= 2 and X.dtype in (torch.complex128, torch.complex64)
    n1, n2 = int(X.shape[-2]), int(n2)
    assert int(X.shape[-1]) == n2 // 2 + 1, f"irfft2d_batch: the last dimension must hold n2//2 + 1 = {n2 // 2 + 1} bins, got {X.shape[-1]}"
    rdt = torch.float64 if X.dtype == torch.complex128 else torch.float32
    shape = tuple(X.shape[:-1]) + (n2,)
    if out is None:
        out = torch.empty(shape, dtype=rdt, device=X.device)
    assert tuple(out.shape) == shape and out.dtype == rdt and out.device == X.device and out.is_contiguous(), \
        f"out must be a contiguous {rdt} tensor of shape {shape} on {X.device}"
    batch = math.prod(int(v) for v in X.shape[:-2])
    with torch.cuda.device(X.device):
        L.check(L.load().dfft_rfft2d_batch(X.data_ptr(), out.data_ptr(), n1, n2, batch, F64 if rdt == torch.float64 else F32, BACKWARD,
                                           None), "dfft_rfft2d_batch")
        torch.cuda.synchronize()
    return out


def fft2d_batch(x, direction: int = FORWARD, out=None):
    """2D FFT of every (n1, n2) plane of a (batch, n1, n2) complex device tensor -- the t0 stage of a 3D plan as a call of its own
    (dfft_fft2d_batch; templateFFT's FFTDim = 2 application, templateFFT.cpp:5767).  out=x transforms in place."""
    import torch
    assert x.is_cuda and x.is_contiguous() and x.dim() == 3
    out = _check_out(x, out)
    with torch.cuda.device(x.device):
        L.check(L.load().dfft_fft2d_batch(x.data_ptr(), out.data_ptr(), x.shape[1], x.shape[2], x.shape[0], _dtype_code(x), direction,
                                          None), "dfft_fft2d_batch")
        torch.cuda.synchronize()
        L.check(L.load().dfft_fft2d_batch_status(None), "dfft_fft2d_batch")  # a one-launch stage that gave up: reported on this call
    return out
