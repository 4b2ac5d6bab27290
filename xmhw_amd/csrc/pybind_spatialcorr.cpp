// pybind_spatialcorr.cpp -- the bindings of spatial_correlation() (include/xmhw_amd.h, "spatial_correlation()"), in a
// module of their own for the reason pybind_stress.cpp gives: the surface of _xmhw_hip is pinned name for name by recorded
// fixtures ("Entry layer").  Same rules as pybind.cpp: no logic, a binding's body is one call of its C entry.
// The exceptions raised are the classes of _xmhw_hip.
#include "pybind_common.h"

PYBIND11_MODULE(_xmhw_hip_spatialcorr, m) {
    m.doc() = "C-ABI bindings of spatial_correlation(): the integer sums of per-cell correlation with grid neighbours";
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

    m.attr("SPATIAL_CORR_MAX_OFFSETS") = XMHW_SPATIAL_CORR_MAX_OFFSETS;
    m.attr("SPATIAL_CORR_REACH") = XMHW_SPATIAL_CORR_REACH;
    m.attr("SPATIAL_CORR_MAX_CLASSES") = XMHW_SPATIAL_CORR_MAX_CLASSES;
    m.attr("SPATIAL_CORR_MAX_STEPS") = XMHW_SPATIAL_CORR_MAX_STEPS;
    m.attr("SPATIAL_CORR_MAX_AXIS") = XMHW_SPATIAL_CORR_MAX_AXIS;
    m.attr("SPATIAL_CORR_BITS") = XMHW_SPATIAL_CORR_BITS;
    m.attr("SPATIAL_CORR_RANGE_BITS") = XMHW_SPATIAL_CORR_RANGE_BITS;
    m.attr("SPATIAL_CORR_MAX_SHIFT") = XMHW_SPATIAL_CORR_MAX_SHIFT;
    m.def("set_spatial_corr_block", [](int steps) { check(xmhw_set_spatial_corr_block(steps)); }, py::arg("steps"));
    m.def("set_spatial_corr_tile", [](int rows) { check(xmhw_set_spatial_corr_tile(rows)); }, py::arg("rows"));
    m.def("spatial_corr_init", [](int32_t K, int32_t D, int32_t ny, int32_t nx, Ptr n, Ptr sx, Ptr sy, Ptr sxx, Ptr syy,
                                  Ptr sxy, int64_t ldo, Ptr n_range, Ptr stream) {
        check(xmhw_spatial_corr_init(K, D, ny, nx, n, sx, sy, sxx, syy, sxy, ldo, n_range, stream));
    }, py::arg("K"), py::arg("D"), py::arg("ny"), py::arg("nx"), py::arg("n"), py::arg("sx"), py::arg("sy"), py::arg("sxx"),
       py::arg("syy"), py::arg("sxy"), py::arg("ldo"), py::arg("n_range"), py::arg("stream") = 0);
    m.def("spatial_corr_accumulate", [](Ptr ts, int itemsize, int64_t ld, int64_t t0, int64_t nt, int64_t T, int32_t ny,
                                        int32_t nx, int32_t periodic, Ptr base, int64_t ldb, int64_t Dr, i32arr row_of_t,
                                        int32_t shift, i32arr class_of_t, int32_t K, i32arr offsets, Ptr n, Ptr sx, Ptr sy,
                                        Ptr sxx, Ptr syy, Ptr sxy, int64_t ldo, Ptr n_range, Ptr stream) {
        check_length(row_of_t, T, "row_of_t");
        check_length(class_of_t, T, "class_of_t");
        if (offsets.ndim() != 2 || offsets.shape(1) != 2) throw InvalidError("offsets must be (D, 2)");
        const int32_t D = static_cast<int32_t>(std::min<py::ssize_t>(offsets.shape(0), INT32_MAX));
        py::gil_scoped_release r;
        check(by_itemsize(itemsize, xmhw_spatial_corr_accumulate_f32, xmhw_spatial_corr_accumulate_f64, ts, ld, t0, nt, T, ny,
                          nx, periodic, base, ldb, Dr, row_of_t.data(), shift, class_of_t.data(), K, offsets.data(), D, n, sx,
                          sy, sxx, syy, sxy, ldo, n_range, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("ld"), py::arg("t0"), py::arg("nt"), py::arg("T"), py::arg("ny"),
       py::arg("nx"), py::arg("periodic"), py::arg("base"), py::arg("ldb"), py::arg("Dr"), py::arg("row_of_t"),
       py::arg("shift"), py::arg("class_of_t"), py::arg("K"), py::arg("offsets"), py::arg("n"), py::arg("sx"), py::arg("sy"),
       py::arg("sxx"), py::arg("syy"), py::arg("sxy"), py::arg("ldo"), py::arg("n_range"), py::arg("stream") = 0);
}
