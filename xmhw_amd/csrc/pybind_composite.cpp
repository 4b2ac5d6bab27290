// pybind_composite.cpp -- the bindings of mhw_composite() (include/xmhw_amd.h, "mhw_composite()"), in a module of their
// own for the reason pybind_stress.cpp gives: the surface of _xmhw_hip is pinned name for name by recorded fixtures
// ("Entry layer").  Same rules as pybind.cpp: no logic, a binding's body is one call of its C entry.  The
// exceptions raised are the classes of _xmhw_hip.
#include "pybind_common.h"

PYBIND11_MODULE(_xmhw_hip_composite, m) {
    m.doc() = "C-ABI bindings of mhw_composite(): the integer sums of event-centred composites";
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

    m.attr("COMPOSITE_MAX_OFFSETS") = XMHW_COMPOSITE_MAX_OFFSETS;
    m.attr("COMPOSITE_MAX_CLASSES") = XMHW_COMPOSITE_MAX_CLASSES;
    m.attr("COMPOSITE_MAX_STEPS") = XMHW_COMPOSITE_MAX_STEPS;
    m.attr("COMPOSITE_BITS") = XMHW_COMPOSITE_BITS;
    m.attr("COMPOSITE_RANGE_BITS") = XMHW_COMPOSITE_RANGE_BITS;
    m.attr("COMPOSITE_MAX_SHIFT") = XMHW_COMPOSITE_MAX_SHIFT;
    m.def("set_composite_block", [](int steps) { check(xmhw_set_composite_block(steps)); }, py::arg("steps"));
    m.def("composite_init", [](int32_t K, int32_t D, int64_t C, Ptr n, Ptr s, Ptr ss, int64_t ldo, Ptr n_range, Ptr stream) {
        check(xmhw_composite_init(K, D, C, n, s, ss, ldo, n_range, stream));
    }, py::arg("K"), py::arg("D"), py::arg("C"), py::arg("n"), py::arg("s"), py::arg("ss"), py::arg("ldo"), py::arg("n_range"),
       py::arg("stream") = 0);
    m.def("composite_accumulate", [](Ptr ts, int itemsize, int64_t T, int64_t C, int64_t ld, Ptr base, int64_t ldb, int64_t Dr,
                                     i32arr row_of_t, int32_t shift, Ptr anchor_bits, int64_t lda, i32arr class_of_t,
                                     int32_t K, int32_t before, int32_t after, Ptr n, Ptr s, Ptr ss, int64_t ldo, Ptr n_range,
                                     Ptr stream) {
        check_length(row_of_t, T, "row_of_t");
        check_length(class_of_t, T, "class_of_t");
        py::gil_scoped_release r;
        check(by_itemsize(itemsize, xmhw_composite_accumulate_f32, xmhw_composite_accumulate_f64, ts, T, C, ld, base, ldb, Dr,
                          row_of_t.data(), shift, anchor_bits, lda, class_of_t.data(), K, before, after, n, s, ss, ldo, n_range,
                          stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("base"), py::arg("ldb"),
       py::arg("Dr"), py::arg("row_of_t"), py::arg("shift"), py::arg("anchor_bits"), py::arg("lda"), py::arg("class_of_t"),
       py::arg("K"), py::arg("before"), py::arg("after"), py::arg("n"), py::arg("s"), py::arg("ss"), py::arg("ldo"),
       py::arg("n_range"), py::arg("stream") = 0);
}
