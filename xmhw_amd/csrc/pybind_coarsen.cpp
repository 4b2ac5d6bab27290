// pybind_coarsen.cpp -- the bindings of coarsen() (include/xmhw_amd.h, "coarsen()"), in a module of their own for the
// reason pybind_stress.cpp gives: the surface of _xmhw_hip is pinned name for name by recorded fixtures ("Entry
// layer").  Same rules as pybind.cpp: no logic, a binding's body is one call of its C entry.  The exceptions raised are the
// classes of _xmhw_hip.
#include "pybind_common.h"

PYBIND11_MODULE(_xmhw_hip_coarsen, m) {
    m.doc() = "C-ABI bindings of coarsen(): weighted block means in space and time";
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

    m.attr("COARSEN_MAX_VOLUME") = XMHW_COARSEN_MAX_VOLUME;
    m.attr("COARSEN_MAX_WEIGHT_BITS") = XMHW_COARSEN_MAX_WEIGHT_BITS;
    m.attr("COARSEN_BITS") = XMHW_REGION_SERIES_BITS;
    m.def("set_coarsen_variant", [](int variant) { check(xmhw_set_coarsen_variant(variant)); }, py::arg("variant"));
    m.def("set_coarsen_chunk", [](int windows) { check(xmhw_set_coarsen_chunk(windows)); }, py::arg("windows"));
    m.def("coarsen_class", [](Ptr ts, Ptr wi, int64_t ld, int32_t nx, int32_t itemsize, int32_t fx) {
        return xmhw_coarsen_class(ts, wi, ld, nx, itemsize, fx);
    }, py::arg("ts"), py::arg("wi"), py::arg("ld"), py::arg("nx"), py::arg("itemsize"), py::arg("fx"));
    m.def("coarsen", [](Ptr ts, int itemsize, int64_t nt, int64_t ld, int32_t ny, int32_t nx, int32_t fy, int32_t fx,
                        int32_t ncy, int32_t ncx, Ptr wi, double x0, int32_t a, i32arr win, Ptr out, int64_t ldo, Ptr wsum,
                        Ptr n, Ptr n_range, Ptr stream) {
        if (win.ndim() != 1 || win.size() < 1) throw InvalidError("win must hold ns + 1 boundaries");
        const int32_t ns = static_cast<int32_t>(std::min<py::ssize_t>(win.size() - 1, INT32_MAX));
        py::gil_scoped_release r;
        check(by_itemsize(itemsize, xmhw_coarsen_f32, xmhw_coarsen_f64, ts, nt, ld, ny, nx, fy, fx, ncy, ncx, wi, x0, a,
                          win.data(), ns, out, ldo, wsum, n, n_range, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("nt"), py::arg("ld"), py::arg("ny"), py::arg("nx"), py::arg("fy"),
       py::arg("fx"), py::arg("ncy"), py::arg("ncx"), py::arg("wi"), py::arg("x0"), py::arg("a"), py::arg("win"),
       py::arg("out"), py::arg("ldo"), py::arg("wsum") = 0, py::arg("n") = 0, py::arg("n_range") = 0, py::arg("stream") = 0);
}
