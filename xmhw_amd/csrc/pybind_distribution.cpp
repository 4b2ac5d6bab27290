// pybind_distribution.cpp -- the bindings of anomaly_distribution() (include/xmhw_amd.h, "anomaly_distribution()"), in a
// module of their own for the reason pybind_stress.cpp gives: the surface of _xmhw_hip is pinned name for name by recorded
// fixtures ("Entry layer").  Same rules as pybind.cpp: no logic, a binding's body is one call of its C entry.
// The exceptions raised are the classes of _xmhw_hip.
#include "pybind_common.h"

using u64arr = py::array_t<uint64_t, py::array::c_style | py::array::forcecast>;

PYBIND11_MODULE(_xmhw_hip_distribution, m) {
    m.doc() = "C-ABI bindings of anomaly_distribution(): per-cell histograms, power sums and extremes of the anomaly";
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

    m.attr("DISTRIBUTION_MAX_BINS") = XMHW_DISTRIBUTION_MAX_BINS;
    m.attr("DISTRIBUTION_MAX_CLASSES") = XMHW_DISTRIBUTION_MAX_CLASSES;
    m.attr("DISTRIBUTION_MAX_QUANTILES") = XMHW_DISTRIBUTION_MAX_QUANTILES;
    m.attr("DISTRIBUTION_MAX_LEVELS") = XMHW_DISTRIBUTION_MAX_LEVELS;
    m.attr("DISTRIBUTION_MAX_STEPS") = XMHW_DISTRIBUTION_MAX_STEPS;
    m.attr("DISTRIBUTION_BITS") = XMHW_DISTRIBUTION_BITS;
    m.attr("DISTRIBUTION_RANGE_BITS") = XMHW_DISTRIBUTION_RANGE_BITS;
    m.attr("DISTRIBUTION_MAX_SHIFT") = XMHW_DISTRIBUTION_MAX_SHIFT;
    m.def("set_distribution_block", [](int steps) { check(xmhw_set_distribution_block(steps)); }, py::arg("steps"));
    m.def("distribution_init", [](int32_t K, int32_t B, int64_t C, Ptr hist, Ptr n, Ptr s1, Ptr s2, Ptr s3, Ptr s4, Ptr kmin,
                                  Ptr kmax, int64_t ldo, Ptr n_range, Ptr stream) {
        check(xmhw_distribution_init(K, B, C, hist, n, s1, s2, s3, s4, kmin, kmax, ldo, n_range, stream));
    }, py::arg("K"), py::arg("B"), py::arg("C"), py::arg("hist"), py::arg("n"), py::arg("s1"), py::arg("s2"), py::arg("s3"),
       py::arg("s4"), py::arg("kmin"), py::arg("kmax"), py::arg("ldo"), py::arg("n_range"), py::arg("stream") = 0);
    m.def("distribution_accumulate", [](Ptr ts, int itemsize, int64_t T, int64_t C, int64_t ld, Ptr base, int64_t ldb,
                                        int64_t Dr, i32arr row_of_t, int32_t shift, i32arr class_of_t, int32_t K, int64_t lo_q,
                                        int32_t width_q, int32_t B, Ptr hist, Ptr n, Ptr s1, Ptr s2, Ptr s3, Ptr s4, Ptr kmin,
                                        Ptr kmax, int64_t ldo, Ptr n_range, Ptr stream) {
        check_length(row_of_t, T, "row_of_t");
        check_length(class_of_t, T, "class_of_t");
        py::gil_scoped_release r;
        check(by_itemsize(itemsize, xmhw_distribution_accumulate_f32, xmhw_distribution_accumulate_f64, ts, T, C, ld, base, ldb,
                          Dr, row_of_t.data(), shift, class_of_t.data(), K, lo_q, width_q, B, hist, n, s1, s2, s3, s4, kmin,
                          kmax, ldo, n_range, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("base"), py::arg("ldb"),
       py::arg("Dr"), py::arg("row_of_t"), py::arg("shift"), py::arg("class_of_t"), py::arg("K"), py::arg("lo_q"),
       py::arg("width_q"), py::arg("B"), py::arg("hist"), py::arg("n"), py::arg("s1"), py::arg("s2"), py::arg("s3"),
       py::arg("s4"), py::arg("kmin"), py::arg("kmax"), py::arg("ldo"), py::arg("n_range"), py::arg("stream") = 0);
    m.def("distribution_finish", [](int32_t K, int32_t B, int64_t C, Ptr hist, Ptr n, Ptr kmin, Ptr kmax, u64arr p_q,
                                    i32arr edge, Ptr qbin, Ptr qbelow, Ptr qcount, Ptr n_at_least, int64_t ldo,
                                    Ptr stream) {
        check(xmhw_distribution_finish(K, B, C, hist, n, kmin, kmax, p_q.data(), static_cast<int32_t>(p_q.size()), edge.data(),
                                       static_cast<int32_t>(edge.size()), qbin, qbelow, qcount, n_at_least, ldo, stream));
    }, py::arg("K"), py::arg("B"), py::arg("C"), py::arg("hist"), py::arg("n"), py::arg("kmin"), py::arg("kmax"),
       py::arg("p_q"), py::arg("edge"), py::arg("qbin"), py::arg("qbelow"), py::arg("qcount"), py::arg("n_at_least"),
       py::arg("ldo"), py::arg("stream") = 0);
}
