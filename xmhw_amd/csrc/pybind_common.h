// pybind_common.h -- what the pybind11 modules over the C ABI share (pybind.cpp: _xmhw_hip; pybind_stress.cpp:
// _xmhw_hip_stress): the status -> exception step, the pointer argument, the float dispatch and the label-length check.
// The exception TYPES are per module (anonymous namespace); the Python exception CLASSES exist once, registered by
// _xmhw_hip.
#pragma once
#include <pybind11/numpy.h>
#include <algorithm>
#include <pybind11/pybind11.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/xmhw_amd.h"

namespace py = pybind11;

namespace {

struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };
struct Unsupported : HipError { using HipError::HipError; };       // XMHW_ERR_UNSUPPORTED
struct InvalidError : std::runtime_error { using std::runtime_error::runtime_error; };
struct CommError : std::runtime_error { using std::runtime_error::runtime_error; };

void check(int rc) {
    if (rc == XMHW_OK) return;
    std::string msg = xmhw_last_error();
    if (rc == XMHW_ERR_INVALID) throw InvalidError(msg);
    if (rc == XMHW_ERR_NOMEM) throw std::bad_alloc();
    if (rc == XMHW_ERR_COMM) throw CommError(msg);
    msg += " (code " + std::to_string(rc) + ")";
    if (rc == XMHW_ERR_UNSUPPORTED) throw Unsupported(msg);
    throw HipError(msg);
}

// A device pointer, stream, event, plan or communicator as Python holds it: an integer.  It converts to the pointer type
// of the parameter it is passed for, so one argument list serves the float and the double entry.
struct Ptr {
    uintptr_t value = 0;
    template <typename T>
    operator T*() const { return reinterpret_cast<T*>(value); }
};

// the float32 or the float64 entry on the same arguments -> its status
template <typename F32, typename F64, typename... Args>
int by_itemsize(int itemsize, F32 f32, F64 f64, const Args&... args) {
    if (itemsize == 4) return f32(args...);
    if (itemsize == 8) return f64(args...);
    throw InvalidError("itemsize must be 4 or 8");
}

using i32arr = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;

// row_of_t / class_of_t hold one label per step
void check_length(const i32arr& labels, int64_t T, const char* name) {
    if (labels.size() != T) throw InvalidError(std::string(name) + " length must equal T");
}

}  // namespace

// Ptr loads like the uintptr_t it stands for: the generated signatures, the accepted inputs and the TypeErrors are those
// of an integer argument
namespace pybind11 { namespace detail {
template <>
struct type_caster<Ptr> {
    PYBIND11_TYPE_CASTER(Ptr, make_caster<uintptr_t>::name);
    bool load(handle src, bool convert) {
        make_caster<uintptr_t> as_int;
        if (!as_int.load(src, convert)) return false;
        value.value = cast_op<uintptr_t>(as_int);
        return true;
    }
};
}}  // namespace pybind11::detail
