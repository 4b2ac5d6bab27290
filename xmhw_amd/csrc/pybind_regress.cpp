// pybind_regress.cpp -- the bindings of index_regression() (include/xmhw_amd.h, "index_regression()"), in a module of
// their own for the reason pybind_stress.cpp gives: the surface of _xmhw_hip is pinned name for name by recorded fixtures
// ("Entry layer").  Same rules as pybind.cpp: no logic, a binding's body is one call of its C entry.  The
// exceptions raised are the classes of _xmhw_hip.
#include "pybind_common.h"

PYBIND11_MODULE(_xmhw_hip_regress, m) {
    m.doc() = "C-ABI bindings of index_regression(): the integer sums of lagged regression maps";
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

    m.attr("INDEX_REGRESS_MAX_PREDICTORS") = XMHW_INDEX_REGRESS_MAX_PREDICTORS;
    m.attr("INDEX_REGRESS_MAX_CLASSES") = XMHW_INDEX_REGRESS_MAX_CLASSES;
    m.attr("INDEX_REGRESS_MAX_STEPS") = XMHW_INDEX_REGRESS_MAX_STEPS;
    m.attr("INDEX_REGRESS_BITS") = XMHW_INDEX_REGRESS_BITS;
    m.attr("INDEX_REGRESS_RANGE_BITS") = XMHW_INDEX_REGRESS_RANGE_BITS;
    m.attr("INDEX_REGRESS_PREDICTOR_BITS") = XMHW_INDEX_REGRESS_PREDICTOR_BITS;
    m.def("set_index_regress_block", [](int steps) { check(xmhw_set_index_regress_block(steps)); }, py::arg("steps"));
    m.def("index_regress_init", [](int32_t K, int32_t J, int64_t C, Ptr n, Ptr sa, Ptr saa, Ptr n1, Ptr saa1, Ptr saz, Ptr mz,
                                   Ptr mzz, int64_t ldo, Ptr n_range, Ptr stream) {
        check(xmhw_index_regress_init(K, J, C, n, sa, saa, n1, saa1, saz, mz, mzz, ldo, n_range, stream));
    }, py::arg("K"), py::arg("J"), py::arg("C"), py::arg("n"), py::arg("sa"), py::arg("saa"), py::arg("n1"), py::arg("saa1"),
       py::arg("saz"), py::arg("mz"), py::arg("mzz"), py::arg("ldo"), py::arg("n_range"), py::arg("stream") = 0);
    m.def("index_regress_accumulate", [](Ptr ts, int itemsize, int64_t T, int64_t C, int64_t ld, Ptr base, int64_t ldb,
                                         int64_t D, i32arr row_of_t, i32arr class_of_t, int32_t K, i32arr zq, Ptr n, Ptr sa,
                                         Ptr saa, Ptr n1, Ptr saa1, Ptr saz, Ptr mz, Ptr mzz, int64_t ldo, Ptr n_range,
                                         Ptr stream) {
        check_length(row_of_t, T, "row_of_t");
        check_length(class_of_t, T, "class_of_t");
        if (zq.ndim() != 2 || zq.shape(0) != T) throw InvalidError("zq must be a (T, J) table");
        const int32_t J = static_cast<int32_t>(std::min<py::ssize_t>(zq.shape(1), 0x7FFFFFFF));
        py::gil_scoped_release r;
        check(by_itemsize(itemsize, xmhw_index_regress_accumulate_f32, xmhw_index_regress_accumulate_f64, ts, T, C, ld, base,
                          ldb, D, row_of_t.data(), class_of_t.data(), K, zq.data(), J, n, sa, saa, n1, saa1, saz, mz, mzz, ldo,
                          n_range, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("base"), py::arg("ldb"),
       py::arg("D"), py::arg("row_of_t"), py::arg("class_of_t"), py::arg("K"), py::arg("zq"), py::arg("n"), py::arg("sa"),
       py::arg("saa"), py::arg("n1"), py::arg("saa1"), py::arg("saz"), py::arg("mz"), py::arg("mzz"), py::arg("ldo"),
       py::arg("n_range"), py::arg("stream") = 0);
}
