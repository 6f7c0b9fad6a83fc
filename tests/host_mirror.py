"""What a test needs to call the C++ host mirror (seekstorm_amd/host/host_capi.cpp) through ctypes: the library's path, pointer types
and the C API's structures.  No tests here."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "seekstorm_amd", "lib", "libseekstorm_host.so")
u8p, u16p, u32p, u64p, f32p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint16, C.c_uint32, C.c_uint64, C.c_float))


def P(a, t):
    """a numpy array as a pointer of type t (None stays None)"""
    return None if a is None else a.ctypes.data_as(t)


class SortC(C.Structure):  # ssh_result_sort
    _fields_ = [("facet_offset", C.c_uint32), ("facet_type", C.c_uint32), ("descending", C.c_uint32), ("reserved", C.c_uint32),
                ("base", C.c_double * 2)]
