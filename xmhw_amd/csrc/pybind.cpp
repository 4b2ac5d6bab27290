// pybind.cpp -- thin pybind11 layer over the C ABI (include/xmhw_amd.h).
// No logic lives here: argument unpacking, error code -> exception.  A binding's body is one call of its C entry with the
// lambda's arguments as they are: Ptr turns into whichever pointer the entry declares, by_itemsize picks the float entry.
#include "pybind_common.h"

PYBIND11_MODULE(_xmhw_hip, m) {
    m.doc() = "C-ABI bindings of the gfx950 xmhw threshold() path";
    auto& hip_error = py::register_exception<HipError>(m, "HipError");
    py::register_exception<Unsupported>(m, "Unsupported", hip_error.ptr());
    py::register_exception<InvalidError>(m, "InvalidArgument");
    py::register_exception<CommError>(m, "CommError");

    m.attr("KERNEL_AUTO") = XMHW_KERNEL_AUTO;
    m.attr("KERNEL_RING") = XMHW_KERNEL_RING;
    m.attr("KERNEL_GENERIC") = XMHW_KERNEL_GENERIC;

    m.def("version", &xmhw_version);
    m.def("arch", []() { return std::string(xmhw_arch()); });
    m.def("device_count", []() { int n = 0; check(xmhw_device_count(&n)); return n; });
    m.def("set_device", [](int d) { check(xmhw_set_device(d)); });
    m.def("get_device", []() { int d = 0; check(xmhw_get_device(&d)); return d; });
    m.def("device_info", [](int d) {
        char name[256] = {0};
        int cus = 0;
        uint64_t bytes = 0;
        check(xmhw_device_info(d, name, sizeof(name), &cus, &bytes));
        py::dict r;
        r["name"] = std::string(name);
        r["compute_units"] = cus;
        r["hbm_bytes"] = bytes;
        return r;
    });

    m.def("malloc", [](size_t n) { void* p = nullptr; check(xmhw_malloc(&p, n)); return reinterpret_cast<uintptr_t>(p); });
    m.def("free", [](Ptr p) { check(xmhw_free(p)); });
    m.def("memcpy_h2d", [](Ptr dst, py::buffer src, Ptr stream) {
        py::buffer_info bi = src.request();
        check(xmhw_memcpy_h2d(dst, bi.ptr, static_cast<size_t>(bi.size) * bi.itemsize, stream));
    }, py::arg("dst"), py::arg("src"), py::arg("stream") = 0);
    m.def("memcpy2d_h2d", [](Ptr dst, py::buffer src, int64_t col0, int64_t ncols, Ptr stream) {
        // columns [col0, col0 + ncols) of a C-contiguous 2-D host array -> dense (rows, ncols) device array
        py::buffer_info bi = src.request();
        // rows must be contiguous; the row pitch is free (record variables of a netCDF classic file are
        // interleaved with the other record variables: rows are one record apart)
        if (bi.ndim != 2 || bi.strides[1] != bi.itemsize || bi.strides[0] < bi.itemsize * bi.shape[1])
            throw InvalidError("memcpy2d_h2d needs a 2-D array with contiguous rows");
        if (col0 < 0 || ncols < 0 || col0 + ncols > bi.shape[1]) throw InvalidError("column range outside the array");
        const size_t isz = static_cast<size_t>(bi.itemsize);
        const size_t spitch = static_cast<size_t>(bi.strides[0]);
        py::gil_scoped_release r;
        check(xmhw_memcpy2d_h2d(dst, isz * static_cast<size_t>(ncols), static_cast<const char*>(bi.ptr) + isz * col0,
                                spitch, isz * static_cast<size_t>(ncols), static_cast<size_t>(bi.shape[0]), stream));
    }, py::arg("dst"), py::arg("src"), py::arg("col0"), py::arg("ncols"), py::arg("stream") = 0);
    m.def("memcpy_d2h", [](py::buffer dst, Ptr src, Ptr stream) {
        py::buffer_info bi = dst.request(true);
        py::gil_scoped_release r;        // a large copy must not stall the thread that feeds the next slab
        check(xmhw_memcpy_d2h(bi.ptr, src, static_cast<size_t>(bi.size) * bi.itemsize, stream));
    }, py::arg("dst"), py::arg("src"), py::arg("stream") = 0);
    m.def("memset", [](Ptr dst, int v, size_t n, Ptr stream) { check(xmhw_memset(dst, v, n, stream)); },
          py::arg("dst"), py::arg("value"), py::arg("nbytes"), py::arg("stream") = 0);
    m.def("stream_create", []() { void* s = nullptr; check(xmhw_stream_create(&s)); return reinterpret_cast<uintptr_t>(s); });
    m.def("stream_sync", [](Ptr s) { py::gil_scoped_release r; check(xmhw_stream_sync(s)); }, py::arg("stream") = 0);
    m.def("event_create", []() { void* e = nullptr; check(xmhw_event_create(&e)); return reinterpret_cast<uintptr_t>(e); });
    m.def("event_destroy", [](Ptr e) { check(xmhw_event_destroy(e)); });
    m.def("event_record", [](Ptr e, Ptr s) { check(xmhw_event_record(e, s)); }, py::arg("event"), py::arg("stream") = 0);
    m.def("stream_wait_event", [](Ptr s, Ptr e) { check(xmhw_stream_wait_event(s, e)); });
    m.def("event_elapsed_ms", [](Ptr a, Ptr b) { float ms = 0; check(xmhw_event_elapsed_ms(a, b, &ms)); return ms; });

    m.def("plan_create", [](i32arr doy, int w) {
        xmhw_plan* p = nullptr;
        check(xmhw_plan_create(doy.data(), doy.size(), w, &p));
        return reinterpret_cast<uintptr_t>(p);
    });
    m.def("plan_destroy", [](Ptr p) { check(xmhw_plan_destroy(p)); });
    m.def("plan_info", [](Ptr p) {
        int32_t D, nt, k, ns, smin;
        check(xmhw_plan_info(p, &D, &nt, &k, &ns, &smin));
        py::dict r;
        r["D"] = D; r["ntracks"] = nt; r["kernel"] = k; r["nsteps"] = ns; r["step_min"] = smin;
        return r;
    });
    m.def("plan_doys", [](Ptr p) {
        int32_t D;
        check(xmhw_plan_info(p, &D, nullptr, nullptr, nullptr, nullptr));
        py::array_t<int32_t> out(D);
        check(xmhw_plan_doys(p, out.mutable_data()));
        return out;
    });
    m.def("plan_set_kernel", [](Ptr p, int k) { check(xmhw_plan_set_kernel(p, k)); });
    m.def("plan_set_narrowing", [](Ptr p, int on) { check(xmhw_plan_set_narrowing(p, on)); });
    m.def("plan_narrowed", [](Ptr p) { int32_t n = 0; check(xmhw_plan_narrowed(p, &n)); return n != 0; });
    m.def("plan_set_chunks", [](Ptr p, int n) { check(xmhw_plan_set_chunks(p, n)); });
    m.def("plan_table", [](Ptr p, int yps) {
        int32_t ns, ntp;
        check(xmhw_plan_info(p, nullptr, nullptr, nullptr, &ns, nullptr));
        check(xmhw_plan_table(p, yps, nullptr, &ntp));
        py::array_t<uint32_t> out({static_cast<py::ssize_t>(ns), static_cast<py::ssize_t>(ntp)});
        check(xmhw_plan_table(p, yps, out.mutable_data(), &ntp));
        return out;
    });

    m.def("plan_set_timing", [](Ptr p, int on) { check(xmhw_plan_set_timing(p, on)); });
    m.def("plan_kernel_ms", [](Ptr p, int back) { float ms = 0; check(xmhw_plan_kernel_ms(p, back, &ms)); return ms; });
    m.def("plan_sorted_info", [](Ptr p, int64_t C) {
        int32_t k = 0, lds = 0, pieces = 0;
        check(xmhw_plan_sorted_info(p, C, &k, &lds, &pieces));
        return py::make_tuple(k, lds, pieces);
    });
    m.def("plan_sorted_table", [](Ptr p, int pieces) {
        int32_t nc = 0, nr = 0, ntp = 0;
        check(xmhw_plan_sorted_table(p, pieces, &nc, &nr, &ntp, nullptr, nullptr, nullptr));
        py::array_t<int32_t> chunks({static_cast<py::ssize_t>(nc), static_cast<py::ssize_t>(4)});
        py::array_t<uint32_t> table({static_cast<py::ssize_t>(nr), static_cast<py::ssize_t>(ntp)});
        py::array_t<uint32_t> flags(static_cast<py::ssize_t>(nr));
        check(xmhw_plan_sorted_table(p, pieces, &nc, &nr, &ntp, chunks.mutable_data(), table.mutable_data(),
                                     flags.mutable_data()));
        return py::make_tuple(chunks, table, flags);
    });
    // (an introspection entry behind device.Plan.sorted_direct(); the leading underscore keeps it out of the module's public
    // surface, which tests/golden/binding_signatures.json pins)
    m.def("_plan_sorted_direct", [](Ptr p, int64_t C) { int32_t v = 0; check(xmhw_plan_sorted_direct(p, C, &v)); return v; });

    m.def("plan_debug_stats", [](Ptr p, int enable, bool read) {
        py::array_t<uint64_t> out(16);
        std::fill(out.mutable_data(), out.mutable_data() + 16, uint64_t(0));
        check(xmhw_plan_debug_stats_n(p, enable, read ? out.mutable_data() : nullptr, 16));
        return out;
    });
    m.def("plan_chunks_in_use", [](Ptr p, int64_t C) { int32_t v = 0; check(xmhw_plan_chunks_in_use(p, C, &v)); return v; });
    m.def("debug_stats_available", []() { return xmhw_debug_stats_available() != 0; });
    m.def("plan_set_layout", [](Ptr p, int layout) { check(xmhw_plan_set_layout(p, layout)); });
    m.def("plan_layout_in_use", [](Ptr p) { int32_t v = -1; check(xmhw_plan_layout_in_use(p, &v)); return v; });
    m.def("sorted_device_ok", []() { int32_t v = 0; check(xmhw_sorted_device_ok(&v)); return v != 0; });
    m.def("plan_f64_mode", [](Ptr p) { int32_t v = -1; check(xmhw_plan_f64_mode(p, &v)); return v; });
    m.def("plan_route", [](Ptr p, int elem_bytes, double q, int64_t C) {
        py::array_t<int32_t> out(XMHW_ROUTE_WORDS);
        check(xmhw_plan_route(p, elem_bytes, q, C, out.mutable_data(), XMHW_ROUTE_WORDS));
        return out;
    });

    m.def("clim_raw", [](Ptr plan, Ptr ts, int itemsize, int64_t C, int64_t ld, double q, int negate, Ptr th, Ptr se,
                         int64_t ldo, Ptr stream) {
        check(by_itemsize(itemsize, xmhw_clim_raw_f32, xmhw_clim_raw_f64, plan, ts, C, ld, q, negate, th, se, ldo, stream));
    }, py::arg("plan"), py::arg("ts"), py::arg("itemsize"), py::arg("C"), py::arg("ld"), py::arg("q"),
       py::arg("negate"), py::arg("thresh"), py::arg("seas"), py::arg("ldo"), py::arg("stream") = 0);

    m.def("clim_raw_i16", [](Ptr plan, Ptr codes, int64_t C, int64_t ld, int big_endian, int has_scale, double scale_factor,
                             double add_offset, int has_fill, int32_t fill_code, int decoded_itemsize, double q, int negate,
                             Ptr th, Ptr se, int64_t ldo, Ptr stream) {
        check(xmhw_clim_raw_i16(plan, codes, C, ld, big_endian, has_scale, scale_factor, add_offset, has_fill, fill_code,
                                decoded_itemsize, q, negate, th, se, ldo, stream));
    }, py::arg("plan"), py::arg("codes"), py::arg("C"), py::arg("ld"), py::arg("big_endian"), py::arg("has_scale"),
       py::arg("scale_factor"), py::arg("add_offset"), py::arg("has_fill"), py::arg("fill_code"), py::arg("decoded_itemsize"),
       py::arg("q"), py::arg("negate"), py::arg("thresh"), py::arg("seas"), py::arg("ldo"), py::arg("stream") = 0);

    m.def("clim_finish", [](Ptr plan, Ptr th_in, Ptr se_in, int64_t C, int64_t ldo, int feb29_fix, int smooth, int width,
                            Ptr th_out, Ptr se_out, Ptr stream) {
        check(xmhw_clim_finish(plan, th_in, se_in, C, ldo, feb29_fix, smooth, width, th_out, se_out, stream));
    }, py::arg("plan"), py::arg("thresh_in"), py::arg("seas_in"), py::arg("C"), py::arg("ldo"),
       py::arg("feb29_fix"), py::arg("smooth"), py::arg("width"), py::arg("thresh_out"), py::arg("seas_out"),
       py::arg("stream") = 0);

    m.def("clim_host", [](py::array ts, i32arr doy, int D, int w, double q, int smooth, int smooth_w, int feb29_fix,
                          int negate) {
        if (ts.ndim() != 2) throw InvalidError("ts must be (T, C)");
        if (!(ts.flags() & py::array::c_style)) throw InvalidError("ts must be C-contiguous");
        if (ts.shape(0) != doy.size()) throw InvalidError("doy length must equal T");
        const int64_t T = ts.shape(0), C = ts.shape(1);
        py::array_t<double> th({static_cast<py::ssize_t>(D), static_cast<py::ssize_t>(C)});
        py::array_t<double> se({static_cast<py::ssize_t>(D), static_cast<py::ssize_t>(C)});
        int rc;
        if (ts.dtype().is(py::dtype::of<float>())) {
            py::gil_scoped_release r;
            rc = xmhw_clim_host_f32(static_cast<const float*>(ts.data()), doy.data(), T, C, D, w, q, smooth, smooth_w,
                                    feb29_fix, negate, th.mutable_data(), se.mutable_data());
        } else if (ts.dtype().is(py::dtype::of<double>())) {
            py::gil_scoped_release r;
            rc = xmhw_clim_host_f64(static_cast<const double*>(ts.data()), doy.data(), T, C, D, w, q, smooth, smooth_w,
                                    feb29_fix, negate, th.mutable_data(), se.mutable_data());
        } else {
            throw InvalidError("ts dtype must be float32 or float64");
        }
        check(rc);
        return py::make_tuple(th, se);
    });

    m.def("land_mask", [](Ptr ts, int itemsize, int64_t T, int64_t C, int64_t ld, int anynans, Ptr keep, Ptr stream) {
        check(by_itemsize(itemsize, xmhw_land_mask_f32, xmhw_land_mask_f64, ts, T, C, ld, anynans, keep, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("anynans"),
       py::arg("keep"), py::arg("stream") = 0);
    m.def("land_mask_i16", [](Ptr codes, int64_t T, int64_t C, int64_t ld, int big_endian, int has_fill, int32_t fill_code,
                              int anynans, Ptr keep, Ptr stream) {
        check(xmhw_land_mask_i16(codes, T, C, ld, big_endian, has_fill, fill_code, anynans, keep, stream));
    }, py::arg("codes"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("big_endian"), py::arg("has_fill"),
       py::arg("fill_code"), py::arg("anynans"), py::arg("keep"), py::arg("stream") = 0);

    m.def("gather_cells", [](Ptr in, int itemsize, int64_t rows, int64_t ld_in, Ptr index, int64_t n, Ptr out, int64_t ld_out,
                             Ptr stream) {
        // (a third element type: int16 codes are gathered as they are)
        if (itemsize == 2) check(xmhw_gather_cells_i16(in, rows, ld_in, index, n, out, ld_out, stream));
        else if (itemsize == 4) check(xmhw_gather_cells_f32(in, rows, ld_in, index, n, out, ld_out, stream));
        else if (itemsize == 8) check(xmhw_gather_cells_f64(in, rows, ld_in, index, n, out, ld_out, stream));
        else throw InvalidError("itemsize must be 2, 4 or 8");
    }, py::arg("in"), py::arg("itemsize"), py::arg("rows"), py::arg("ld_in"), py::arg("index"), py::arg("n"),
       py::arg("out"), py::arg("ld_out"), py::arg("stream") = 0);
    m.def("scatter_cells", [](Ptr in, int64_t rows, int64_t ld_in, Ptr index, int64_t n, Ptr out, int64_t ld_out, Ptr stream) {
        check(xmhw_scatter_cells_f64(in, rows, ld_in, index, n, out, ld_out, stream));
    }, py::arg("in"), py::arg("rows"), py::arg("ld_in"), py::arg("index"), py::arg("n"), py::arg("out"),
       py::arg("ld_out"), py::arg("stream") = 0);

    m.def("detect_events", [](Ptr ts, int itemsize, int64_t T, int64_t C, int64_t ld, Ptr thresh, int64_t ldt,
                              i32arr row_of_t, int min_duration, int join_gaps, int max_gap, int negate, Ptr events,
                              Ptr start, Ptr end, Ptr bthresh, int64_t ldo, Ptr nevents, Ptr stream) {
        check_length(row_of_t, T, "row_of_t");
        py::gil_scoped_release r;
        check(by_itemsize(itemsize, xmhw_detect_events_f32, xmhw_detect_events_f64, ts, T, C, ld, thresh, ldt, row_of_t.data(),
                          min_duration, join_gaps, max_gap, negate, events, start, end, bthresh, ldo, nevents, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("thresh"), py::arg("ldt"),
       py::arg("row_of_t"), py::arg("min_duration"), py::arg("join_gaps"), py::arg("max_gap"), py::arg("negate"),
       py::arg("events"), py::arg("start"), py::arg("end"), py::arg("bthresh") = 0, py::arg("ldo"), py::arg("nevents") = 0,
       py::arg("stream") = 0);

    m.def("count_events", [](Ptr start, int64_t T, int64_t C, int64_t ldo, Ptr nevents, Ptr stream) {
        check(xmhw_count_events(start, T, C, ldo, nevents, stream));
    }, py::arg("start"), py::arg("T"), py::arg("C"), py::arg("ldo"), py::arg("nevents"), py::arg("stream") = 0);
    m.attr("EVENT_COLUMNS") = XMHW_EVENT_COLUMNS;
    m.def("event_stats", [](Ptr ts, int itemsize, int64_t T, int64_t C, int64_t ld, Ptr seas, Ptr thresh, int64_t ldc,
                            i32arr row_of_t, int negate, Ptr events, int64_t ldo, Ptr offsets, Ptr table, Ptr stream) {
        check_length(row_of_t, T, "row_of_t");
        py::gil_scoped_release r;
        check(by_itemsize(itemsize, xmhw_event_stats_f32, xmhw_event_stats_f64, ts, T, C, ld, seas, thresh, ldc, row_of_t.data(),
                          negate, events, ldo, offsets, table, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("seas"), py::arg("thresh"),
       py::arg("ldc"), py::arg("row_of_t"), py::arg("negate"), py::arg("events"), py::arg("ldo"), py::arg("offsets"),
       py::arg("table"), py::arg("stream") = 0);

    m.def("set_exceed_kernel", [](int mode) { check(xmhw_set_exceed_kernel(mode)); }, py::arg("mode"));
    m.def("exceed_bits", [](Ptr ts, int itemsize, int64_t T, int64_t C, int64_t ld, Ptr thresh, int64_t ldt, int64_t D,
                            i32arr row_of_t, int negate, Ptr bits, int64_t ldb, Ptr stream) {
        check_length(row_of_t, T, "row_of_t");
        py::gil_scoped_release r;
        check(by_itemsize(itemsize, xmhw_exceed_bits_f32, xmhw_exceed_bits_f64, ts, T, C, ld, thresh, ldt, D, row_of_t.data(),
                          negate, bits, ldb, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("thresh"), py::arg("ldt"),
       py::arg("D"), py::arg("row_of_t"), py::arg("negate"), py::arg("bits"), py::arg("ldb"), py::arg("stream") = 0);
    m.def("events_from_bits", [](Ptr bits, int64_t T, int64_t C, int64_t ldb, int min_duration, int join_gaps, int max_gap,
                                 Ptr offsets, Ptr nevents, Ptr table, Ptr stream) {
        check(xmhw_events_from_bits(bits, T, C, ldb, min_duration, join_gaps, max_gap, offsets, nevents, table, stream));
    }, py::arg("bits"), py::arg("T"), py::arg("C"), py::arg("ldb"), py::arg("min_duration"), py::arg("join_gaps"),
       py::arg("max_gap"), py::arg("offsets") = 0, py::arg("nevents") = 0, py::arg("table") = 0, py::arg("stream") = 0);
    m.def("event_stats_sparse", [](Ptr ts, int itemsize, int64_t T, int64_t C, int64_t ld, Ptr seas, Ptr thresh, int64_t ldc,
                                   i32arr row_of_t, int negate, int64_t n_events, Ptr table, Ptr stream) {
        check_length(row_of_t, T, "row_of_t");
        py::gil_scoped_release r;
        check(by_itemsize(itemsize, xmhw_event_stats_sparse_f32, xmhw_event_stats_sparse_f64, ts, T, C, ld, seas, thresh, ldc,
                          row_of_t.data(), negate, n_events, table, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("seas"), py::arg("thresh"),
       py::arg("ldc"), py::arg("row_of_t"), py::arg("negate"), py::arg("n_events"), py::arg("table"), py::arg("stream") = 0);

    m.def("event_intermediate", [](Ptr ts, int itemsize, int64_t T, int64_t C, int64_t ld, Ptr seas, Ptr thresh, int64_t ldc,
                                   i32arr row_of_t, int negate, Ptr events, int64_t ldo, Ptr out, int64_t ldv, Ptr dur,
                                   Ptr stream) {
        check_length(row_of_t, T, "row_of_t");
        py::gil_scoped_release r;
        check(by_itemsize(itemsize, xmhw_event_intermediate_f32, xmhw_event_intermediate_f64, ts, T, C, ld, seas, thresh, ldc,
                          row_of_t.data(), negate, events, ldo, out, ldv, dur, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("seas"), py::arg("thresh"),
       py::arg("ldc"), py::arg("row_of_t"), py::arg("negate"), py::arg("events"), py::arg("ldo"), py::arg("out"),
       py::arg("ldv"), py::arg("dur"), py::arg("stream") = 0);

    // ---- sharded path: RCCL communicator + the one gather ---------------------------------
    m.def("comm_unique_id", []() {
        std::string id(XMHW_UNIQUE_ID_BYTES, '\0');
        check(xmhw_comm_unique_id(&id[0]));
        return py::bytes(id);
    });
    m.def("comm_create", [](int rank, int nranks, py::bytes id) {
        std::string sid = id;
        if (sid.size() != XMHW_UNIQUE_ID_BYTES) throw InvalidError("unique id must be 128 bytes");
        xmhw_comm* c = nullptr;
        {
            py::gil_scoped_release r;
            check(xmhw_comm_create(rank, nranks, sid.data(), &c));
        }
        return reinterpret_cast<uintptr_t>(c);
    });
    m.def("comm_destroy", [](Ptr c) { check(xmhw_comm_destroy(c)); });
    m.def("comm_allgather_i64", [](Ptr c, int64_t value, Ptr stream) {
        int rank = 0, n = 0;
        check(xmhw_comm_info(c, &rank, &n));
        py::array_t<int64_t> out(n);
        {
            py::gil_scoped_release r;
            check(xmhw_comm_allgather_i64(c, value, out.mutable_data(), stream));
        }
        return out;
    }, py::arg("comm"), py::arg("value"), py::arg("stream") = 0);
    m.def("comm_allgather_bytes", [](Ptr c, Ptr send, Ptr recv, size_t n, Ptr stream) {
        check(xmhw_comm_allgather_bytes(c, send, recv, n, stream));
    }, py::arg("comm"), py::arg("send"), py::arg("recv"), py::arg("bytes_per_rank"), py::arg("stream") = 0);
    m.def("gather_blocks", [](Ptr c, Ptr send, int64_t rows, int64_t cols, Ptr recv,
                              py::array_t<int64_t, py::array::c_style | py::array::forcecast> cols_of_rank, int root,
                              Ptr stream) {
        check(xmhw_gather_blocks(c, send, rows, cols, recv, cols_of_rank.size() ? cols_of_rank.data() : nullptr, root, stream));
    }, py::arg("comm"), py::arg("send"), py::arg("rows"), py::arg("cols"), py::arg("recv"), py::arg("cols_of_rank"),
       py::arg("root") = 0, py::arg("stream") = 0);
    m.def("memcpy2d_d2h", [](py::buffer dst, int64_t col0, int64_t ncols, Ptr src, Ptr stream) {
        // dense (rows, ncols) device array -> columns [col0, col0 + ncols) of a C-contiguous 2-D host array
        py::buffer_info bi = dst.request(true);
        if (bi.ndim != 2 || bi.strides[1] != bi.itemsize || bi.strides[0] != bi.itemsize * bi.shape[1])
            throw InvalidError("memcpy2d_d2h needs a C-contiguous 2-D array");
        if (col0 < 0 || ncols < 0 || col0 + ncols > bi.shape[1]) throw InvalidError("column range outside the array");
        const size_t isz = static_cast<size_t>(bi.itemsize);
        py::gil_scoped_release r;
        check(xmhw_memcpy2d_d2h(static_cast<char*>(bi.ptr) + isz * col0, isz * static_cast<size_t>(bi.shape[1]), src,
                                isz * static_cast<size_t>(ncols), isz * static_cast<size_t>(ncols),
                                static_cast<size_t>(bi.shape[0]), stream));
    }, py::arg("dst"), py::arg("col0"), py::arg("ncols"), py::arg("src"), py::arg("stream") = 0);
    m.def("memcpy2d_d2h_async", [](py::buffer dst, int64_t col0, int64_t ncols, Ptr src, Ptr stream) {
        // dense (rows, ncols) device array -> columns [col0, col0 + ncols) of a C-contiguous 2-D host array
        py::buffer_info bi = dst.request(true);
        if (bi.ndim != 2 || bi.strides[1] != bi.itemsize || bi.strides[0] != bi.itemsize * bi.shape[1])
            throw InvalidError("memcpy2d_d2h_async needs a C-contiguous 2-D array");
        if (col0 < 0 || ncols < 0 || col0 + ncols > bi.shape[1]) throw InvalidError("column range outside the array");
        const size_t isz = static_cast<size_t>(bi.itemsize);
        py::gil_scoped_release r;
        check(xmhw_memcpy2d_d2h_async(static_cast<char*>(bi.ptr) + isz * col0, isz * static_cast<size_t>(bi.shape[1]), src,
                                      isz * static_cast<size_t>(ncols), isz * static_cast<size_t>(ncols),
                                      static_cast<size_t>(bi.shape[0]), stream));
    }, py::arg("dst"), py::arg("col0"), py::arg("ncols"), py::arg("src"), py::arg("stream") = 0);

    m.def("decode", [](Ptr raw, int raw_itemsize, int big_endian, int64_t rows, int64_t cols, int64_t ld_raw, Ptr out,
                       int out_itemsize, int64_t ld_out, bool has_scale, double scale, double offset, bool has_fill,
                       double fill, Ptr stream) {
        check(xmhw_decode(raw, raw_itemsize, big_endian, rows, cols, ld_raw, out, out_itemsize, ld_out, has_scale, scale,
                          offset, has_fill, fill, stream));
    }, py::arg("raw"), py::arg("raw_itemsize"), py::arg("big_endian"), py::arg("rows"), py::arg("cols"), py::arg("ld_raw"),
       py::arg("out"), py::arg("out_itemsize"), py::arg("ld_out"), py::arg("has_scale"), py::arg("scale"),
       py::arg("offset"), py::arg("has_fill"), py::arg("fill"), py::arg("stream") = 0);
    m.def("encode_i16", [](Ptr in, int64_t rows, int64_t cols, int64_t ld_in, Ptr out, int64_t ld_out, double scale,
                           double offset, int32_t fill, Ptr stream) {
        check(xmhw_encode_i16(in, rows, cols, ld_in, out, ld_out, scale, offset, fill, stream));
    }, py::arg("in"), py::arg("rows"), py::arg("cols"), py::arg("ld_in"), py::arg("out"), py::arg("ld_out"), py::arg("scale"),
       py::arg("offset"), py::arg("fill"), py::arg("stream") = 0);
    m.def("read_rows", [](int fd, int64_t off, int64_t pitch, int64_t row_bytes, int64_t rows, Ptr dst) {
        py::gil_scoped_release r;
        int rc = xmhw_read_rows(fd, off, pitch, row_bytes, rows, dst);
        py::gil_scoped_acquire a;
        check(rc);
    }, py::arg("fd"), py::arg("file_offset"), py::arg("row_pitch"), py::arg("row_bytes"), py::arg("rows"), py::arg("dst"));
    m.def("pad_gaps", [](Ptr ts, int itemsize, int64_t T, int64_t C, int64_t ld, Ptr x, double max_gap, Ptr stream) {
        check(xmhw_pad_gaps(ts, itemsize, T, C, ld, x, max_gap, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("x"), py::arg("max_gap"),
       py::arg("stream") = 0);
    m.def("host_alloc", [](size_t n) { void* p = nullptr; check(xmhw_host_alloc(&p, n)); return reinterpret_cast<uintptr_t>(p); });
    m.def("host_free", [](Ptr p) { check(xmhw_host_free(p)); });
    m.def("host_view", [](Ptr p, size_t nbytes) {
        // a numpy uint8 view of page-locked memory obtained from host_alloc (the caller keeps it alive)
        const uint8_t* bytes = p;
        return py::array_t<uint8_t>({nbytes}, {1}, bytes, py::none());
    });
    m.def("memcpy_h2d_async", [](Ptr dst, Ptr src, size_t bytes, Ptr stream) {
        check(xmhw_memcpy_h2d_async(dst, src, bytes, stream));
    });
    m.def("event_sync", [](Ptr e) { py::gil_scoped_release r; check(xmhw_event_sync(e)); });

    m.def("block_events", [](Ptr table, Ptr offsets, int64_t C, Ptr bin_of_t, int64_t T, int nbins, int mtime_col, Ptr out,
                             int64_t ldo, Ptr stream) {
        check(xmhw_block_events(table, offsets, C, bin_of_t, T, nbins, mtime_col, out, ldo, stream));
    }, py::arg("table"), py::arg("offsets"), py::arg("C"), py::arg("bin_of_t"), py::arg("T"), py::arg("nbins"),
       py::arg("mtime_col"), py::arg("out"), py::arg("ldo"), py::arg("stream") = 0);
    m.def("event_rank", [](Ptr table, int64_t ld_table, Ptr offsets, int64_t C, py::sequence cols, double n_years, Ptr rank,
                           Ptr rp, int64_t ld_out, Ptr stream) {
        std::vector<int32_t> columns;
        for (auto c : cols) columns.push_back(c.cast<int32_t>());
        check(xmhw_event_rank(table, ld_table, offsets, C, columns.data(), static_cast<int32_t>(columns.size()), n_years, rank,
                              rp, ld_out, stream));
    }, py::arg("table"), py::arg("ld_table"), py::arg("offsets"), py::arg("C"), py::arg("columns"), py::arg("n_years"),
       py::arg("rank"), py::arg("rp"), py::arg("ld_out"), py::arg("stream") = 0);
    m.attr("COVERAGE_MAX_REGIONS") = XMHW_COVERAGE_MAX_REGIONS;
    m.attr("COVERAGE_STATES") = XMHW_COVERAGE_STATES;
    m.def("coverage_accumulate", [](Ptr ts, int itemsize, int64_t T, int64_t C, int64_t ld, Ptr seas, Ptr thresh, int64_t ldc,
                                    i32arr row_of_t, int negate, Ptr bits, int64_t ldb, int min_duration, int join_gaps,
                                    int max_gap, Ptr wq, Ptr region, int32_t R, Ptr cells, Ptr area_q, Ptr stream) {
        check_length(row_of_t, T, "row_of_t");
        py::gil_scoped_release r;
        check(by_itemsize(itemsize, xmhw_coverage_accumulate_f32, xmhw_coverage_accumulate_f64, ts, T, C, ld, seas, thresh, ldc,
                          row_of_t.data(), negate, bits, ldb, min_duration, join_gaps, max_gap, wq, region, R, cells, area_q,
                          stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("seas"), py::arg("thresh"),
       py::arg("ldc"), py::arg("row_of_t"), py::arg("negate"), py::arg("bits"), py::arg("ldb"), py::arg("min_duration"),
       py::arg("join_gaps"), py::arg("max_gap"), py::arg("wq"), py::arg("region"), py::arg("R"), py::arg("cells"),
       py::arg("area_q"), py::arg("stream") = 0);
    m.attr("REGION_MAX_REGIONS") = XMHW_REGION_MAX_REGIONS;
    m.attr("REGION_SERIES_BITS") = XMHW_REGION_SERIES_BITS;
    m.def("set_region_wave_sum", [](int variant) { check(xmhw_set_region_wave_sum(variant)); }, py::arg("variant"));
    m.def("region_accumulate", [](Ptr ts, int itemsize, int64_t T, int64_t C, int64_t ld, double x0, Ptr wi, Ptr region,
                                  int32_t R, Ptr acc, Ptr n_range, Ptr stream) {
        py::gil_scoped_release r;
        check(by_itemsize(itemsize, xmhw_region_accumulate_f32, xmhw_region_accumulate_f64, ts, T, C, ld, x0, wi, region, R, acc,
                          n_range, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("x0"), py::arg("wi"),
       py::arg("region"), py::arg("R"), py::arg("acc"), py::arg("n_range"), py::arg("stream") = 0);
    m.def("event_objects", [](Ptr start, Ptr end, int64_t n, Ptr offsets, int64_t C, Ptr nbr, int32_t K, int32_t gap,
                              Ptr cell_of_row, Ptr root, Ptr stream) {
        check(xmhw_event_objects(start, end, n, offsets, C, nbr, K, gap, cell_of_row, root, stream));
    }, py::arg("start"), py::arg("end"), py::arg("n"), py::arg("offsets"), py::arg("C"), py::arg("nbr"), py::arg("K"),
       py::arg("gap"), py::arg("cell_of_row"), py::arg("root"), py::arg("stream") = 0);
    m.def("object_reduce", [](Ptr start, Ptr end, Ptr imax, int64_t n, Ptr cell_of_row, Ptr offsets, Ptr wq, Ptr slot,
                              int64_t n_slots, Ptr n_events, Ptr n_cells, Ptr time_start, Ptr time_end, Ptr cell_days,
                              Ptr area_days_q, Ptr intensity_max, Ptr peak_row, Ptr stream) {
        check(xmhw_object_reduce(start, end, imax, n, cell_of_row, offsets, wq, slot, n_slots, n_events, n_cells, time_start,
                                 time_end, cell_days, area_days_q, intensity_max, peak_row, stream));
    }, py::arg("start"), py::arg("end"), py::arg("imax"), py::arg("n"), py::arg("cell_of_row"), py::arg("offsets"),
       py::arg("wq"), py::arg("slot"), py::arg("n_slots"), py::arg("n_events"), py::arg("n_cells"), py::arg("time_start"),
       py::arg("time_end"), py::arg("cell_days"), py::arg("area_days_q"), py::arg("intensity_max"), py::arg("peak_row"),
       py::arg("stream") = 0);
    m.def("object_tracks", [](Ptr start, Ptr end, int64_t n, Ptr slot, Ptr cell_of_row, int64_t C, Ptr vec, int64_t ldv,
                              Ptr time_start, Ptr offsets, int64_t n_slots, int64_t L, Ptr n_cells, Ptr sums, int64_t ld,
                              Ptr n_bad, Ptr stream) {
        check(xmhw_object_tracks(start, end, n, slot, cell_of_row, C, vec, ldv, time_start, offsets, n_slots, L, n_cells, sums,
                                 ld, n_bad, stream));
    }, py::arg("start"), py::arg("end"), py::arg("n"), py::arg("slot"), py::arg("cell_of_row"), py::arg("C"), py::arg("vec"),
       py::arg("ldv"), py::arg("time_start"), py::arg("offsets"), py::arg("n_slots"), py::arg("L"), py::arg("n_cells"),
       py::arg("sums"), py::arg("ld"), py::arg("n_bad"), py::arg("stream") = 0);
    m.def("object_parts", [](Ptr start, Ptr end, Ptr slot, Ptr cell_of_row, int64_t n, Ptr row_offsets, int64_t C, Ptr nbr,
                             int32_t K, Ptr wq, Ptr vox_off, int64_t V, Ptr time_start, Ptr offsets, int64_t n_slots,
                             int64_t L, Ptr n_parts, Ptr cells_largest, Ptr area_largest_q, Ptr n_bad, Ptr stream) {
        check(xmhw_object_parts(start, end, slot, cell_of_row, n, row_offsets, C, nbr, K, wq, vox_off, V, time_start, offsets,
                                n_slots, L, n_parts, cells_largest, area_largest_q, n_bad, stream));
    }, py::arg("start"), py::arg("end"), py::arg("slot"), py::arg("cell_of_row"), py::arg("n"), py::arg("row_offsets"),
       py::arg("C"), py::arg("nbr"), py::arg("K"), py::arg("wq"), py::arg("vox_off"), py::arg("V"), py::arg("time_start"),
       py::arg("offsets"), py::arg("n_slots"), py::arg("L"), py::arg("n_parts"), py::arg("cells_largest"),
       py::arg("area_largest_q"), py::arg("n_bad"), py::arg("stream") = 0);
    m.def("object_genealogy", [](Ptr start, Ptr end, Ptr slot, Ptr cell_of_row, int64_t n, Ptr row_offsets, int64_t C, Ptr nbr,
                                 int32_t K, Ptr vox_off, int64_t V, Ptr time_start, Ptr offsets, int64_t n_slots, int64_t L,
                                 Ptr counts, Ptr edges, int64_t edge_capacity, Ptr n_edges, Ptr n_bad, Ptr overflow,
                                 Ptr stream) {
        check(xmhw_object_genealogy(start, end, slot, cell_of_row, n, row_offsets, C, nbr, K, vox_off, V, time_start, offsets,
                                    n_slots, L, counts, edges, edge_capacity, n_edges, n_bad, overflow, stream));
    }, py::arg("start"), py::arg("end"), py::arg("slot"), py::arg("cell_of_row"), py::arg("n"), py::arg("row_offsets"),
       py::arg("C"), py::arg("nbr"), py::arg("K"), py::arg("vox_off"), py::arg("V"), py::arg("time_start"),
       py::arg("offsets"), py::arg("n_slots"), py::arg("L"), py::arg("counts"), py::arg("edges"), py::arg("edge_capacity"),
       py::arg("n_edges"), py::arg("n_bad"), py::arg("overflow"), py::arg("stream") = 0);
    m.def("object_shape", [](Ptr start, Ptr end, Ptr slot, Ptr cell_of_row, int64_t n, Ptr row_offsets, int64_t C, Ptr faces,
                             int32_t K, Ptr lq, Ptr time_start, Ptr offsets, int64_t n_slots, int64_t L, Ptr edges,
                             Ptr perimeter_q, Ptr cells_edge, Ptr n_bad, Ptr stream) {
        check(xmhw_object_shape(start, end, slot, cell_of_row, n, row_offsets, C, faces, K, lq, time_start, offsets, n_slots, L,
                                edges, perimeter_q, cells_edge, n_bad, stream));
    }, py::arg("start"), py::arg("end"), py::arg("slot"), py::arg("cell_of_row"), py::arg("n"), py::arg("row_offsets"),
       py::arg("C"), py::arg("faces"), py::arg("K"), py::arg("lq"), py::arg("time_start"), py::arg("offsets"),
       py::arg("n_slots"), py::arg("L"), py::arg("edges"), py::arg("perimeter_q"), py::arg("cells_edge"), py::arg("n_bad"),
       py::arg("stream") = 0);
    m.attr("SHAPE_CLASSES") = XMHW_SHAPE_CLASSES;
    m.attr("SHAPE_FACE_COAST") = XMHW_SHAPE_FACE_COAST;
    m.attr("SHAPE_FACE_BORDER") = XMHW_SHAPE_FACE_BORDER;
    m.attr("SHAPE_FACE_FOLDED") = XMHW_SHAPE_FACE_FOLDED;
    m.attr("GENEALOGY_VOXEL_BYTES") = XMHW_GENEALOGY_VOXEL_BYTES;
    m.attr("GENEALOGY_SLOT_BYTES") = XMHW_GENEALOGY_SLOT_BYTES;
    m.attr("GENEALOGY_FIELDS") = XMHW_GENEALOGY_FIELDS;
    m.attr("PARTS_VOXEL_BYTES") = XMHW_PARTS_VOXEL_BYTES;
    m.attr("TRACKS_TILE") = XMHW_TRACKS_TILE;
    m.attr("TRACK_INTENSITY_CHUNK") = XMHW_TRACK_INTENSITY_CHUNK;
    m.attr("TRACK_INTENSITY_BITS") = XMHW_TRACK_INTENSITY_BITS;
    m.def("set_track_intensity_combine", [](int on) { check(xmhw_set_track_intensity_combine(on)); }, py::arg("on"));
    m.def("track_intensity_init", [](int64_t L, Ptr n_valid, Ptr wsum_i, Ptr isum_q, Ptr intensity_max, Ptr cat_cells,
                                     int64_t ldcat, Ptr n_range, Ptr n_bad, Ptr stream) {
        check(xmhw_track_intensity_init(L, n_valid, wsum_i, isum_q, intensity_max, cat_cells, ldcat, n_range, n_bad, stream));
    }, py::arg("L"), py::arg("n_valid"), py::arg("wsum_i"), py::arg("isum_q"), py::arg("intensity_max"), py::arg("cat_cells"),
       py::arg("ldcat"), py::arg("n_range"), py::arg("n_bad"), py::arg("stream") = 0);
    m.def("track_intensity_accumulate", [](Ptr ts, int itemsize, int64_t T, int64_t n, int64_t ld, Ptr seas, Ptr thresh,
                                           int64_t ldc, int64_t D, i32arr row_of_t, int negate, Ptr start, Ptr end, Ptr slot,
                                           int64_t n_rows, Ptr row_offsets, Ptr wi, Ptr time_start, Ptr offsets,
                                           int64_t n_slots, int64_t L, Ptr n_valid, Ptr wsum_i, Ptr isum_q, Ptr intensity_max,
                                           Ptr cat_cells, int64_t ldcat, Ptr n_range, Ptr n_bad, Ptr stream) {
        check_length(row_of_t, T, "row_of_t");
        py::gil_scoped_release r;
        check(by_itemsize(itemsize, xmhw_track_intensity_accumulate_f32, xmhw_track_intensity_accumulate_f64, ts, T, n, ld, seas,
                          thresh, ldc, D, row_of_t.data(), negate, start, end, slot, n_rows, row_offsets, wi, time_start,
                          offsets, n_slots, L, n_valid, wsum_i, isum_q, intensity_max, cat_cells, ldcat, n_range, n_bad,
                          stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("T"), py::arg("n"), py::arg("ld"), py::arg("seas"), py::arg("thresh"),
       py::arg("ldc"), py::arg("D"), py::arg("row_of_t"), py::arg("negate"), py::arg("start"), py::arg("end"), py::arg("slot"),
       py::arg("n_rows"), py::arg("row_offsets"), py::arg("wi"), py::arg("time_start"), py::arg("offsets"), py::arg("n_slots"),
       py::arg("L"), py::arg("n_valid"), py::arg("wsum_i"), py::arg("isum_q"), py::arg("intensity_max"), py::arg("cat_cells"),
       py::arg("ldcat"), py::arg("n_range"), py::arg("n_bad"), py::arg("stream") = 0);
    m.def("track_intensity_finish", [](int64_t L, Ptr intensity_max, Ptr stream) {
        check(xmhw_track_intensity_finish(L, intensity_max, stream));
    }, py::arg("L"), py::arg("intensity_max"), py::arg("stream") = 0);
    m.attr("CLASS_DAYS_MAX_CLASSES") = XMHW_CLASS_DAYS_MAX_CLASSES;
    m.attr("CLASS_DAYS_CHANNELS") = XMHW_CLASS_DAYS_CHANNELS;
    m.def("set_class_days_block", [](int steps) { check(xmhw_set_class_days_block(steps)); }, py::arg("steps"));
    m.def("class_days_init", [](int32_t K, int64_t C, Ptr days, Ptr isum_q, Ptr intensity_max, int64_t ldo, Ptr n_range,
                                Ptr stream) {
        check(xmhw_class_days_init(K, C, days, isum_q, intensity_max, ldo, n_range, stream));
    }, py::arg("K"), py::arg("C"), py::arg("days"), py::arg("isum_q"), py::arg("intensity_max"), py::arg("ldo"),
       py::arg("n_range"), py::arg("stream") = 0);
    m.def("class_days_accumulate", [](Ptr ts, int itemsize, int64_t T, int64_t C, int64_t ld, Ptr seas, Ptr thresh,
                                      int64_t ldc, i32arr row_of_t, int negate, Ptr bits, int64_t ldb, int min_duration,
                                      int join_gaps, int max_gap, i32arr class_of_t, int32_t K, Ptr days, Ptr isum_q,
                                      Ptr intensity_max, int64_t ldo, Ptr n_range, Ptr stream) {
        check_length(row_of_t, T, "row_of_t");
        check_length(class_of_t, T, "class_of_t");
        py::gil_scoped_release r;
        check(by_itemsize(itemsize, xmhw_class_days_accumulate_f32, xmhw_class_days_accumulate_f64, ts, T, C, ld, seas, thresh,
                          ldc, row_of_t.data(), negate, bits, ldb, min_duration, join_gaps, max_gap, class_of_t.data(), K, days,
                          isum_q, intensity_max, ldo, n_range, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("seas"), py::arg("thresh"),
       py::arg("ldc"), py::arg("row_of_t"), py::arg("negate"), py::arg("bits"), py::arg("ldb"), py::arg("min_duration"),
       py::arg("join_gaps"), py::arg("max_gap"), py::arg("class_of_t"), py::arg("K"), py::arg("days"), py::arg("isum_q"),
       py::arg("intensity_max"), py::arg("ldo"), py::arg("n_range"), py::arg("stream") = 0);
    m.def("class_days_finish", [](int32_t K, int64_t C, Ptr intensity_max, int64_t ldo, Ptr stream) {
        check(xmhw_class_days_finish(K, C, intensity_max, ldo, stream));
    }, py::arg("K"), py::arg("C"), py::arg("intensity_max"), py::arg("ldo"), py::arg("stream") = 0);
    m.attr("COOCCUR_MAX_CLASSES") = XMHW_COOCCUR_MAX_CLASSES;
    m.attr("COOCCUR_MAX_LAGS") = XMHW_COOCCUR_MAX_LAGS;
    m.attr("COOCCUR_CHANNELS") = XMHW_COOCCUR_CHANNELS;
    m.def("event_table_bits", [](Ptr start, Ptr end, Ptr offsets, Ptr cell, int64_t C, int64_t T, Ptr bits, int64_t ldb,
                                 Ptr stream) {
        check(xmhw_event_table_bits(start, end, offsets, cell, C, T, bits, ldb, stream));
    }, py::arg("start"), py::arg("end"), py::arg("offsets"), py::arg("cell"), py::arg("C"), py::arg("T"), py::arg("bits"),
       py::arg("ldb"), py::arg("stream") = 0);
    m.def("set_cooccur_block", [](int words) { check(xmhw_set_cooccur_block(words)); }, py::arg("words"));
    m.def("cooccur_init", [](int32_t K, int32_t L, int64_t C, Ptr counts, int64_t ldo, Ptr stream) {
        check(xmhw_cooccur_init(K, L, C, counts, ldo, stream));
    }, py::arg("K"), py::arg("L"), py::arg("C"), py::arg("counts"), py::arg("ldo"), py::arg("stream") = 0);
    m.def("cooccur_accumulate", [](Ptr a_bits, int64_t lda, Ptr b_bits, int64_t ldb, int64_t T, int64_t C, i32arr class_of_t,
                                   int32_t K, i32arr lags, Ptr counts, int64_t ldo, Ptr stream) {
        check_length(class_of_t, T, "class_of_t");
        const int32_t L = static_cast<int32_t>(lags.size() > 0x7FFFFFFF ? 0x7FFFFFFF : lags.size());
        py::gil_scoped_release r;
        check(xmhw_cooccur_accumulate(a_bits, lda, b_bits, ldb, T, C, class_of_t.data(), K, lags.data(), L, counts, ldo, stream));
    }, py::arg("a_bits"), py::arg("lda"), py::arg("b_bits"), py::arg("ldb"), py::arg("T"), py::arg("C"),
       py::arg("class_of_t"), py::arg("K"), py::arg("lags"), py::arg("counts"), py::arg("ldo"), py::arg("stream") = 0);
    m.attr("DISPLACEMENT_MAX_CLASSES") = XMHW_DISPLACEMENT_MAX_CLASSES;
    m.attr("DISPLACEMENT_MAX_AXIS") = XMHW_DISPLACEMENT_MAX_AXIS;
    m.def("set_displacement_block", [](int steps) { check(xmhw_set_displacement_block(steps)); }, py::arg("steps"));
    m.def("displacement_init", [](int32_t K, int64_t C, Ptr n_days, Ptr n_found, Ptr sum_m, Ptr sum_north_m, Ptr sum_east_m,
                                  Ptr max_m, int64_t ldo, Ptr n_visited, Ptr stream) {
        check(xmhw_displacement_init(K, C, n_days, n_found, sum_m, sum_north_m, sum_east_m, max_m, ldo, n_visited, stream));
    }, py::arg("K"), py::arg("C"), py::arg("n_days"), py::arg("n_found"), py::arg("sum_m"), py::arg("sum_north_m"),
       py::arg("sum_east_m"), py::arg("max_m"), py::arg("ldo"), py::arg("n_visited"), py::arg("stream") = 0);
    m.def("displacement_accumulate", [](Ptr ts, int itemsize, int64_t ld, int64_t t0, int64_t nt, int64_t T, int32_t ny,
                                        int32_t nx, int periodic, Ptr seas, int64_t ldc, int64_t D, i32arr row_of_t,
                                        int negate, Ptr bits, int64_t ldb, Ptr cell_of_point, int64_t C, Ptr basin,
                                        Ptr list_off, Ptr djdi, Ptr dist_m, Ptr north_m, Ptr east_m, int64_t n_entries,
                                        i32arr class_of_t, int32_t K, Ptr n_days, Ptr n_found, Ptr sum_m, Ptr sum_north_m,
                                        Ptr sum_east_m, Ptr max_m, int64_t ldo, Ptr n_visited, Ptr stream) {
        check_length(row_of_t, T, "row_of_t");
        check_length(class_of_t, T, "class_of_t");
        py::gil_scoped_release r;
        check(by_itemsize(itemsize, xmhw_displacement_accumulate_f32, xmhw_displacement_accumulate_f64, ts, ld, t0, nt, T, ny, nx,
                          periodic, seas, ldc, D, row_of_t.data(), negate, bits, ldb, cell_of_point, C, basin, list_off, djdi,
                          dist_m, north_m, east_m, n_entries, class_of_t.data(), K, n_days, n_found, sum_m, sum_north_m,
                          sum_east_m, max_m, ldo, n_visited, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("ld"), py::arg("t0"), py::arg("nt"), py::arg("T"), py::arg("ny"),
       py::arg("nx"), py::arg("periodic"), py::arg("seas"), py::arg("ldc"), py::arg("D"), py::arg("row_of_t"),
       py::arg("negate"), py::arg("bits"), py::arg("ldb"), py::arg("cell_of_point"), py::arg("C"), py::arg("basin"),
       py::arg("list_off"), py::arg("djdi"), py::arg("dist_m"), py::arg("north_m"), py::arg("east_m"), py::arg("n_entries"),
       py::arg("class_of_t"), py::arg("K"), py::arg("n_days"), py::arg("n_found"), py::arg("sum_m"), py::arg("sum_north_m"),
       py::arg("sum_east_m"), py::arg("max_m"), py::arg("ldo"), py::arg("n_visited"), py::arg("stream") = 0);
    m.def("block_trend_ols", [](Ptr y, int32_t nstat, int32_t nb, int64_t C, int64_t ld, Ptr x, Ptr tcrit, Ptr out, int64_t ldo,
                                Ptr stream) {
        check(xmhw_block_trend_ols(y, nstat, nb, C, ld, x, tcrit, out, ldo, stream));
    }, py::arg("y"), py::arg("nstat"), py::arg("nb"), py::arg("C"), py::arg("ld"), py::arg("x"), py::arg("tcrit"),
       py::arg("out"), py::arg("ldo"), py::arg("stream") = 0);
    m.def("block_trend_theil_sen", [](Ptr y, int32_t nstat, int32_t nb, int64_t C, int64_t ld, Ptr x, Ptr out, int64_t ldo,
                                      Ptr stream) {
        check(xmhw_block_trend_theil_sen(y, nstat, nb, C, ld, x, out, ldo, stream));
    }, py::arg("y"), py::arg("nstat"), py::arg("nb"), py::arg("C"), py::arg("ld"), py::arg("x"), py::arg("out"),
       py::arg("ldo"), py::arg("stream") = 0);
    m.attr("FIT_MAX_TERMS") = XMHW_FIT_MAX_TERMS;
    m.def("series_fit", [](Ptr ts, int itemsize, int64_t T, int64_t C, int64_t ld, Ptr basis, int32_t P, Ptr weight,
                           int32_t min_valid, Ptr coef, int64_t ldc, Ptr nvalid, Ptr stream) {
        check(by_itemsize(itemsize, xmhw_series_fit_f32, xmhw_series_fit_f64, ts, T, C, ld, basis, P, weight, min_valid, coef,
                          ldc, nvalid, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("basis"), py::arg("P"),
       py::arg("weight"), py::arg("min_valid"), py::arg("coef"), py::arg("ldc"), py::arg("nvalid") = 0, py::arg("stream") = 0);
    m.def("series_remove", [](Ptr ts, int itemsize, int64_t T, int64_t C, int64_t ld, Ptr basis, int32_t P, int32_t R, Ptr coef,
                              int64_t ldc, Ptr stream) {
        check(by_itemsize(itemsize, xmhw_series_remove_f32, xmhw_series_remove_f64, ts, T, C, ld, basis, P, R, coef, ldc, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("basis"), py::arg("P"),
       py::arg("R"), py::arg("coef"), py::arg("ldc"), py::arg("stream") = 0);
    m.def("block_time", [](Ptr ts, int itemsize, int64_t T, int64_t C, int64_t ld, Ptr cats, int64_t ldcat, Ptr bin_of_t,
                           int nbins, Ptr out, int64_t ldo, Ptr stream) {
        check(by_itemsize(itemsize, xmhw_block_time_f32, xmhw_block_time_f64, ts, T, C, ld, cats, ldcat, bin_of_t, nbins, out,
                          ldo, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("cats"), py::arg("ldcat"),
       py::arg("bin_of_t"), py::arg("nbins"), py::arg("out"), py::arg("ldo"), py::arg("stream") = 0);

    m.def("release_cached_tables", []() { check(xmhw_release_cached_tables()); });
    m.def("offsets_from_counts", [](Ptr counts, int64_t n, Ptr offsets, Ptr stream) {
        check(xmhw_offsets_from_counts(counts, n, offsets, stream));
    }, py::arg("counts"), py::arg("n"), py::arg("offsets"), py::arg("stream") = 0);

    m.def("synth_sst_ex", [](Ptr ts, int64_t T, int64_t C, int64_t ld, int64_t cell0, uint64_t seed, double nan_frac,
                             double quant, double ice_frac, double rho, int64_t ice_patch, Ptr stream) {
        check(xmhw_synth_sst_ex_f32(ts, T, C, ld, cell0, seed, nan_frac, quant, ice_frac, rho, ice_patch, stream));
    }, py::arg("ts"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("cell0"), py::arg("seed"), py::arg("nan_frac") = 0.0,
       py::arg("quant") = 0.0, py::arg("ice_frac") = 0.0, py::arg("rho") = 0.0, py::arg("ice_patch") = 0, py::arg("stream") = 0);
    m.def("synth_sst", [](Ptr ts, int itemsize, int64_t T, int64_t C, int64_t ld, int64_t cell0, uint64_t seed, double nan_frac,
                          Ptr stream) {
        check(by_itemsize(itemsize, xmhw_synth_sst_f32, xmhw_synth_sst_f64, ts, T, C, ld, cell0, seed, nan_frac, stream));
    }, py::arg("ts"), py::arg("itemsize"), py::arg("T"), py::arg("C"), py::arg("ld"), py::arg("cell0"),
       py::arg("seed"), py::arg("nan_frac") = 0.0, py::arg("stream") = 0);
}
