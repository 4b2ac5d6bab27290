// pybind_lagcorr.cpp -- the bindings of lag_correlation() (include/xmhw_amd.h, "lag_correlation()"), in a module of their
// own for the reason pybind_stress.cpp gives: the surface of _xmhw_hip is pinned name for name by recorded fixtures
// ("Entry layer").  Same rules as pybind.cpp: no logic, a binding's body is one call of its C entry.  The
// exceptions raised are the classes of _xmhw_hip.
#include "pybind_common.h"

PYBIND11_MODULE(_xmhw_hip_lagcorr, m) {
    m.doc() = "C-ABI bindings of lag_correlation(): the integer sums of per-cell lagged auto- and cross-correlation";
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

    m.attr("LAG_CORR_MAX_LAG") = XMHW_LAG_CORR_MAX_LAG;
    m.attr("LAG_CORR_MAX_CLASSES") = XMHW_LAG_CORR_MAX_CLASSES;
    m.attr("LAG_CORR_MAX_STEPS") = XMHW_LAG_CORR_MAX_STEPS;
    m.attr("LAG_CORR_BITS") = XMHW_LAG_CORR_BITS;
    m.attr("LAG_CORR_RANGE_BITS") = XMHW_LAG_CORR_RANGE_BITS;
    m.attr("LAG_CORR_MAX_SHIFT") = XMHW_LAG_CORR_MAX_SHIFT;
    m.def("set_lag_corr_block", [](int steps) { check(xmhw_set_lag_corr_block(steps)); }, py::arg("steps"));
    m.def("lag_corr_init", [](int32_t K, int32_t max_lag, int64_t C, Ptr n, Ptr sx, Ptr sy, Ptr sxx, Ptr syy, Ptr sxy,
                              int64_t ldo, Ptr n_range, Ptr stream) {
        check(xmhw_lag_corr_init(K, max_lag, C, n, sx, sy, sxx, syy, sxy, ldo, n_range, stream));
    }, py::arg("K"), py::arg("max_lag"), py::arg("C"), py::arg("n"), py::arg("sx"), py::arg("sy"), py::arg("sxx"),
       py::arg("syy"), py::arg("sxy"), py::arg("ldo"), py::arg("n_range"), py::arg("stream") = 0);
    m.def("lag_corr_accumulate", [](Ptr x, int64_t ldx, Ptr y, int64_t ldy, int itemsize, int64_t T, int64_t C, Ptr base_x,
                                    int64_t ldbx, Ptr base_y, int64_t ldby, int64_t Dr, i32arr row_of_t, int32_t shift_x,
                                    int32_t shift_y, i32arr class_of_t, int32_t K, int32_t max_lag, Ptr n, Ptr sx, Ptr sy,
                                    Ptr sxx, Ptr syy, Ptr sxy, int64_t ldo, Ptr n_range, Ptr stream) {
        check_length(row_of_t, T, "row_of_t");
        check_length(class_of_t, T, "class_of_t");
        py::gil_scoped_release r;
        check(by_itemsize(itemsize, xmhw_lag_corr_accumulate_f32, xmhw_lag_corr_accumulate_f64, x, ldx, y, ldy, T, C, base_x,
                          ldbx, base_y, ldby, Dr, row_of_t.data(), shift_x, shift_y, class_of_t.data(), K, max_lag, n, sx, sy,
                          sxx, syy, sxy, ldo, n_range, stream));
    }, py::arg("x"), py::arg("ldx"), py::arg("y"), py::arg("ldy"), py::arg("itemsize"), py::arg("T"), py::arg("C"),
       py::arg("base_x"), py::arg("ldbx"), py::arg("base_y"), py::arg("ldby"), py::arg("Dr"), py::arg("row_of_t"),
       py::arg("shift_x"), py::arg("shift_y"), py::arg("class_of_t"), py::arg("K"), py::arg("max_lag"), py::arg("n"),
       py::arg("sx"), py::arg("sy"), py::arg("sxx"), py::arg("syy"), py::arg("sxy"), py::arg("ldo"), py::arg("n_range"),
       py::arg("stream") = 0);
}
