// pybind_regrid.cpp -- the bindings of regrid() (include/xmhw_amd.h, "regrid()"), in a module of their own for the
// reason pybind_stress.cpp gives: the surface of _xmhw_hip is pinned name for name by recorded fixtures ("Entry
// layer").  Same rules as pybind.cpp: no logic, a binding's body is one call of its C entry (after the lengths of the host
// tables have been checked against my and mx: the C entry cannot see them).  The exceptions raised are the classes of
// _xmhw_hip.
#include "pybind_common.h"

namespace {

// first[m], ptr[m + 1], full[m]; weights[] long enough for the entries the pointer table names
void check_axis(const i32arr& first, const i32arr& ptr, const i32arr& weights, const i32arr& full, const char* name) {
    const py::ssize_t m = first.size();
    if (first.ndim() != 1 || ptr.ndim() != 1 || weights.ndim() != 1 || full.ndim() != 1 || m > INT32_MAX - 1 ||
        ptr.size() != m + 1 || full.size() != m || weights.size() < ptr.data()[m])
        throw InvalidError(std::string("the ") + name + " tables must be first[m], ptr[m + 1], weights[ptr[m]] and full[m]");
}

}  // namespace

PYBIND11_MODULE(_xmhw_hip_regrid, m) {
    m.doc() = "C-ABI bindings of regrid(): conservative remapping between lat-lon grids";
    // the exception classes exist once, in _xmhw_hip: this module's C++ exceptions are translated to them
    const py::module_ core = py::module_::import("xmhw_amd._xmhw_hip");
    static PyObject* const hip_error = py::object(core.attr("HipError")).release().ptr();
    static PyObject* const unsupported = py::object(core.attr("Unsupported")).release().ptr();
    static PyObject* const invalid = py::object(core.attr("InvalidArgument")).release().ptr();
    static PyObject* const comm = py::object(core.attr("CommError")).release().ptr();
    py::register_local_exception_translator([](std::exception_ptr p) {
        try {
            if (p) std::rethrow_exception(p);
        } catch (const Unsupported& e) {
            PyErr_SetString(unsupported, e.what());
        } catch (const HipError& e) {
            PyErr_SetString(hip_error, e.what());
        } catch (const InvalidError& e) {
            PyErr_SetString(invalid, e.what());
        } catch (const CommError& e) {
            PyErr_SetString(comm, e.what());
        }
    });

    m.attr("REGRID_MAX_RUN") = XMHW_REGRID_MAX_RUN;
    m.attr("REGRID_MAX_WEIGHT") = XMHW_REGRID_MAX_WEIGHT;
    m.attr("REGRID_MAX_EXTENT") = XMHW_REGRID_MAX_EXTENT;
    m.attr("REGRID_BITS") = XMHW_REGION_SERIES_BITS;
    m.def("set_regrid_variant", [](int variant) { check(xmhw_set_regrid_variant(variant)); }, py::arg("variant"));
    m.def("set_regrid_chunk", [](int steps) { check(xmhw_set_regrid_chunk(steps)); }, py::arg("steps"));
    m.def("regrid_class", [](int32_t nx, i32arr row_ptr, i32arr col_first, i32arr col_ptr, int32_t periodic) {
        if (row_ptr.ndim() != 1 || row_ptr.size() < 1 || col_first.ndim() != 1 || col_ptr.ndim() != 1 ||
            col_ptr.size() != col_first.size() + 1 || col_ptr.size() > INT32_MAX)
            throw InvalidError("the tables must be row_ptr[my + 1], col_first[mx] and col_ptr[mx + 1]");
        return xmhw_regrid_class(nx, static_cast<int32_t>(std::min<py::ssize_t>(row_ptr.size() - 1, INT32_MAX)),
                                 static_cast<int32_t>(col_first.size()), row_ptr.data(), col_first.data(), col_ptr.data(), periodic);
    }, py::arg("nx"), py::arg("row_ptr"), py::arg("col_first"), py::arg("col_ptr"), py::arg("periodic"));
    m.def("regrid", [](Ptr ts, int itemsize, int64_t nt, int64_t ld, int32_t ny, int32_t nx, i32arr row_first, i32arr row_ptr,
                       i32arr ay, i32arr wy, i32arr col_first, i32arr col_ptr, i32arr ax, i32arr wx, int32_t periodic, double x0,
                       int32_t a, Ptr out, int64_t ldo, Ptr wsum, Ptr n, Ptr n_range, Ptr stream) {
        check_axis(row_first, row_ptr, ay, wy, "row");
        check_axis(col_first, col_ptr, ax, wx, "column");
        const int32_t my = static_cast<int32_t>(row_first.size()), mx = static_cast<int32_t>(col_first.size());
        py::gil_scoped_release r;
        check(by_itemsize(itemsize, xmhw_regrid_f32, xmhw_regrid_f64, ts, nt, ld, ny, nx, my, mx, row_first.data(), row_ptr.data(),
                          ay.data(), wy.data(), col_first.data(), col_ptr.data(), ax.data(), wx.data(), periodic, x0, a, out, ldo,
                          wsum, n, n_range, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("nt"), py::arg("ld"), py::arg("ny"), py::arg("nx"), py::arg("row_first"),
       py::arg("row_ptr"), py::arg("ay"), py::arg("wy"), py::arg("col_first"), py::arg("col_ptr"), py::arg("ax"), py::arg("wx"),
       py::arg("periodic"), py::arg("x0"), py::arg("a"), py::arg("out"), py::arg("ldo"), py::arg("wsum") = 0, py::arg("n") = 0,
       py::arg("n_range") = 0, py::arg("stream") = 0);
}
