// pybind_stress.cpp -- the bindings of heat_stress() (include/xmhw_amd.h, "heat_stress()"), in a module of their own:
// the surface of _xmhw_hip is pinned name for name by recorded fixtures (tests/test_host_binding_signatures.py), and
// these move there when the fixtures are next re-recorded ("Entry layer").  Same rules as pybind.cpp: no logic,
// a binding's body is one call of its C entry.  The exceptions raised are the classes of _xmhw_hip.
#include "pybind_common.h"

namespace {

using i64arr = py::array_t<int64_t, py::array::c_style | py::array::forcecast>;

// the length of a small host table as the int32 its entry takes (an over-long one is refused there)
int32_t table_length(py::ssize_t n) { return static_cast<int32_t>(n > 0x7FFFFFFF ? 0x7FFFFFFF : n); }

}  // namespace

PYBIND11_MODULE(_xmhw_hip_stress, m) {
    m.doc() = "C-ABI bindings of heat_stress(): class sums of the series and accumulated thermal stress";
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

    m.attr("HEAT_STRESS_MAX_CLASSES") = XMHW_HEAT_STRESS_MAX_CLASSES;
    m.attr("HEAT_STRESS_CHANNELS") = XMHW_HEAT_STRESS_CHANNELS;
    m.attr("HEAT_STRESS_MAX_LEVELS") = XMHW_HEAT_STRESS_MAX_LEVELS;
    m.attr("HEAT_STRESS_MAX_SNAPSHOTS") = XMHW_HEAT_STRESS_MAX_SNAPSHOTS;
    m.attr("HEAT_STRESS_MAX_WINDOW") = XMHW_HEAT_STRESS_MAX_WINDOW;
    m.attr("HEAT_STRESS_BITS") = XMHW_HEAT_STRESS_BITS;
    m.def("set_heat_stress_block", [](int steps) { check(xmhw_set_heat_stress_block(steps)); }, py::arg("steps"));
    m.def("class_sums_init", [](int32_t K, int64_t C, Ptr n_valid, Ptr sum_q, int64_t ldo, Ptr n_range, Ptr stream) {
        check(xmhw_class_sums_init(K, C, n_valid, sum_q, ldo, n_range, stream));
    }, py::arg("K"), py::arg("C"), py::arg("n_valid"), py::arg("sum_q"), py::arg("ldo"), py::arg("n_range"),
       py::arg("stream") = 0);
    m.def("class_sums_accumulate", [](Ptr ts, int itemsize, int64_t T, int64_t C, int64_t ld, double x0, i32arr class_of_t,
                                      int32_t K, Ptr n_valid, Ptr sum_q, int64_t ldo, Ptr n_range, Ptr stream) {
        check_length(class_of_t, T, "class_of_t");
        py::gil_scoped_release r;
        check(by_itemsize(itemsize, xmhw_class_sums_accumulate_f32, xmhw_class_sums_accumulate_f64, ts, T, C, ld, x0,
                          class_of_t.data(), K, n_valid, sum_q, ldo, n_range, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("x0"), py::arg("class_of_t"),
       py::arg("K"), py::arg("n_valid"), py::arg("sum_q"), py::arg("ldo"), py::arg("n_range"), py::arg("stream") = 0);
    m.def("heat_stress_init", [](int32_t K, int64_t C, Ptr counts, Ptr hsum_q, Ptr peak_key, int64_t ldo, Ptr n_range,
                                 Ptr stream) {
        check(xmhw_heat_stress_init(K, C, counts, hsum_q, peak_key, ldo, n_range, stream));
    }, py::arg("K"), py::arg("C"), py::arg("counts"), py::arg("hsum_q"), py::arg("peak_key"), py::arg("ldo"),
       py::arg("n_range"), py::arg("stream") = 0);
    m.def("heat_stress_accumulate", [](Ptr ts, int itemsize, int64_t T, int64_t C, int64_t ld, Ptr base, int64_t ldb,
                                       int64_t D, i32arr row_of_t, int negate, int32_t W, double h0, i32arr class_of_t,
                                       int32_t K, i64arr level_q, i32arr at, Ptr counts, Ptr hsum_q, Ptr peak_key,
                                       Ptr snap_q, int64_t ldo, Ptr n_range, Ptr stream) {
        check_length(row_of_t, T, "row_of_t");
        check_length(class_of_t, T, "class_of_t");
        const int32_t L = table_length(level_q.size()), J = table_length(at.size());
        py::gil_scoped_release r;
        check(by_itemsize(itemsize, xmhw_heat_stress_accumulate_f32, xmhw_heat_stress_accumulate_f64, ts, T, C, ld, base, ldb, D,
                          row_of_t.data(), negate, W, h0, class_of_t.data(), K, level_q.data(), L, at.data(), J, counts,
                          hsum_q, peak_key, snap_q, ldo, n_range, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("base"), py::arg("ldb"),
       py::arg("D"), py::arg("row_of_t"), py::arg("negate"), py::arg("W"), py::arg("h0"), py::arg("class_of_t"), py::arg("K"),
       py::arg("level_q"), py::arg("at"), py::arg("counts"), py::arg("hsum_q"), py::arg("peak_key"), py::arg("snap_q"),
       py::arg("ldo"), py::arg("n_range"), py::arg("stream") = 0);
    m.def("heat_stress_finish", [](int32_t K, int64_t C, Ptr peak_key, Ptr peak_q, Ptr peak_t, int64_t ldo, Ptr stream) {
        check(xmhw_heat_stress_finish(K, C, peak_key, peak_q, peak_t, ldo, stream));
    }, py::arg("K"), py::arg("C"), py::arg("peak_key"), py::arg("peak_q"), py::arg("peak_t"), py::arg("ldo"),
       py::arg("stream") = 0);
}
