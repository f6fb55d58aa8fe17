// pybind11 bindings of the native runtime: module ``mipipe._runtime``.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <stdexcept>

#include "../common/rrc.hpp"
#include "runtime.hpp"

namespace py = pybind11;
using namespace mipipe_rt;

PYBIND11_MODULE(_runtime, m) {
  m.doc() = "mipipe native runtime: process supervisor, DAG scheduler, record loader";

  py::class_<ProcessGroup>(m, "ProcessGroup")
      .def(py::init<bool>(), py::arg("echo") = true)
      .def("spawn", &ProcessGroup::spawn, py::arg("argv"), py::arg("env"), py::arg("cwd") = "",
           py::arg("log_path") = "", py::arg("prefix") = "")
      .def("wait", &ProcessGroup::wait, py::arg("timeout") = 0.0, py::arg("grace") = 10.0,
           py::call_guard<py::gil_scoped_release>())
      .def("signal_all", &ProcessGroup::signal_all)
      .def("interrupt", &ProcessGroup::interrupt)
      .def("exit_codes", &ProcessGroup::exit_codes)
      .def("pids", &ProcessGroup::pids)
      .def_property_readonly("failed_rank", &ProcessGroup::failed_rank);

  py::class_<DagScheduler> d(m, "DagScheduler");
  d.def(py::init<int, const std::vector<std::vector<int>>&, const std::vector<bool>&, bool>(),
        py::arg("n"), py::arg("deps"), py::arg("always_run"), py::arg("fail_fast") = true)
      .def("next_ready", &DagScheduler::next_ready)
      .def("complete", &DagScheduler::complete)
      .def("take_cancelled", &DagScheduler::take_cancelled)
      .def("mark_external_failure", &DagScheduler::mark_external_failure)
      .def("finished", &DagScheduler::finished)
      .def("deadlocked", &DagScheduler::deadlocked)
      .def("states", &DagScheduler::states)
      .def("topo_order", &DagScheduler::topo_order);
  d.attr("PENDING") = (int)DagScheduler::kPending;
  d.attr("RUNNING") = (int)DagScheduler::kRunning;
  d.attr("SUCCEEDED") = (int)DagScheduler::kSucceeded;
  d.attr("CACHED") = (int)DagScheduler::kCached;
  d.attr("SKIPPED") = (int)DagScheduler::kSkipped;
  d.attr("FAILED") = (int)DagScheduler::kFailed;
  d.attr("CANCELLED") = (int)DagScheduler::kCancelled;

  py::class_<LoaderConfig>(m, "LoaderConfig")
      .def(py::init<>())
      .def_readwrite("files", &LoaderConfig::files)
      .def_readwrite("header_bytes", &LoaderConfig::header_bytes)
      .def_readwrite("label_bytes", &LoaderConfig::label_bytes)
      .def_readwrite("C", &LoaderConfig::C)
      .def_readwrite("H", &LoaderConfig::H)
      .def_readwrite("W", &LoaderConfig::W)
      .def_readwrite("batch", &LoaderConfig::batch)
      .def_readwrite("train", &LoaderConfig::train)
      .def_readwrite("pad", &LoaderConfig::pad)
      .def_readwrite("flip", &LoaderConfig::flip)
      .def_readwrite("mean", &LoaderConfig::mean)
      .def_readwrite("std", &LoaderConfig::stdv)
      .def_readwrite("seed", &LoaderConfig::seed)
      .def_readwrite("workers", &LoaderConfig::workers)
      .def_readwrite("prefetch", &LoaderConfig::prefetch)
      .def_readwrite("drop_last", &LoaderConfig::drop_last)
      .def_readwrite("raw", &LoaderConfig::raw)
      .def_readwrite("transform", &LoaderConfig::transform)
      .def_readwrite("out_h", &LoaderConfig::out_h)
      .def_readwrite("out_w", &LoaderConfig::out_w)
      .def_readwrite("auto_augment", &LoaderConfig::auto_augment)
      .def_readwrite("erase_pq", &LoaderConfig::erase_pq);

  // the "rrc" transform's geometry (csrc/common/rrc.hpp), for tests against the Python definition
  m.def("rrc_box",
        [](uint64_t seed, uint64_t epoch, uint64_t index, int H, int W, bool train, bool flip) {
          if (H < 2 || W < 2 || H > 32768 || W > 32768)
            throw std::invalid_argument("rrc_box needs H, W in [2, 32768]");
          const mipipe_rrc::Box b = mipipe_rrc::rrc_box(seed, epoch, index, H, W, train, flip);
          return py::make_tuple(b.y0, b.x0, b.h, b.w, b.flip);
        },
        py::arg("seed"), py::arg("epoch"), py::arg("index"), py::arg("H"), py::arg("W"),
        py::arg("train"), py::arg("flip") = true);
  m.def("rrc_ratio_q16", [] {
    std::vector<uint32_t> v(mipipe_rrc::kRatios);
    for (int t = 0; t < mipipe_rrc::kRatios; ++t) v[t] = mipipe_rrc::ratio_q16(t);
    return v;
  });

  py::class_<RecordLoader>(m, "RecordLoader")
      .def(py::init<const LoaderConfig&>())
      .def("__len__", &RecordLoader::size)
      .def("size", &RecordLoader::size)
      .def("start_epoch", &RecordLoader::start_epoch, py::call_guard<py::gil_scoped_release>())
      .def("batches_per_epoch", &RecordLoader::batches_per_epoch)
      // x_ptr / y_ptr: addresses of caller-owned (pinned) host buffers large enough for a batch
      .def("next_into",
           [](RecordLoader& l, uintptr_t x, uintptr_t y) {
             return l.next(reinterpret_cast<float*>(x), reinterpret_cast<int64_t*>(y));
           },
           py::call_guard<py::gil_scoped_release>())
      .def("record_bytes", &RecordLoader::record_bytes)
      // raw mode: rec_ptr [batch, record_bytes] uint8 and idx_ptr [batch] int64 host buffers
      .def("next_raw_into",
           [](RecordLoader& l, uintptr_t rec, uintptr_t idx) {
             return l.next_raw(reinterpret_cast<uint8_t*>(rec), reinterpret_cast<int64_t*>(idx));
           },
           py::call_guard<py::gil_scoped_release>());
}
