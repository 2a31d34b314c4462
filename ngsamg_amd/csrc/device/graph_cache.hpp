// Captured applications, keyed by what identifies one (the vector addresses): at most MAX_GRAPHS, the oldest capture goes
// first, the hot ones stay.  One cache serves the single-rank handle (Handle::graphs), the multi-vector state (MultiState::graphs)
// and the communicator's whole-cycle graph (Comm::graphs).
#pragma once
#include <exception>
#include <map>
#include <string>
#include <vector>
#include "launch.hpp"

namespace amgx {

struct NoPayload {};

template <class Key, class Payload = NoPayload>
struct GraphCache {
  static constexpr size_t MAX_GRAPHS = 16;
  struct Entry { hipGraphExec_t exec; Payload payload; };   // payload: what the owner keeps per capture (Comm: its number of exchanges)
  // why a capture did not work out: the step that failed with its error, or what the body threw
  struct Failure {
    const char* step = nullptr;
    hipError_t err = hipSuccess;
    std::exception_ptr thrown;
    std::string text() const {
      if (thrown) { try { std::rethrow_exception(thrown); } catch (const std::exception& ex) { return ex.what(); } catch (...) { return "unknown exception"; } }
      return hipGetErrorString(err);
    }
    [[noreturn]] void raise() const {
      if (thrown) std::rethrow_exception(thrown);
      throw Err(std::string(step) + " failed: " + hipGetErrorString(err));
    }
  };

  std::map<Key, Entry> graphs;
  std::vector<Key> age;                 // capture order
  GraphCache() = default;
  GraphCache(const GraphCache&) = delete;
  GraphCache& operator=(const GraphCache&) = delete;
  ~GraphCache() { drop(); }
  void drop() {
    for (auto& g : graphs) (void)hipGraphExecDestroy(g.second.exec);
    graphs.clear();
    age.clear();
  }
  size_t size() const { return graphs.size(); }
  bool has(const Key& key) const { return graphs.count(key) != 0; }
  Entry* find(const Key& key) { auto it = graphs.find(key); return it == graphs.end() ? nullptr : &it->second; }

  // Captures body() on `stream` in the caller's capture mode and keeps the instantiated graph under `key`.  Never throws for
  // a capture that does not work out: returns nullptr with `why` filled, the stream is out of capture mode again and the cache
  // is as before.  The caller launches the entry (and fills its payload).
  template <class Body>
  Entry* capture(const Key& key, hipStream_t stream, hipStreamCaptureMode mode, Body&& body, Failure& why) {
    why = Failure{};
    if ((why.err = hipStreamBeginCapture(stream, mode)) != hipSuccess) { why.step = "hipStreamBeginCapture"; (void)hipGetLastError(); return nullptr; }
    try { body(); } catch (...) { why.thrown = std::current_exception(); }
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    why.err = hipStreamEndCapture(stream, &g);
    if (why.thrown) why.step = "capture body";
    else if (why.err != hipSuccess || !g) why.step = "hipStreamEndCapture";
    else if ((why.err = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0)) != hipSuccess) why.step = "hipGraphInstantiate";
    if (g) (void)hipGraphDestroy(g);
    if (why.step) { (void)hipGetLastError(); return nullptr; }
    if (graphs.size() >= MAX_GRAPHS && !age.empty()) {      // the oldest capture goes, the hot ones stay
      auto old = graphs.find(age.front());
      age.erase(age.begin());
      if (old != graphs.end()) { (void)hipGraphExecDestroy(old->second.exec); graphs.erase(old); }
    }
    age.push_back(key);
    return &graphs.emplace(key, Entry{ge, Payload{}}).first->second;
  }

  // replays the graph of `key`; the first call with a key captures body() on `stream` (thread-local capture; a capture that
  // fails throws)
  template <class Body>
  void run(const Key& key, hipStream_t stream, Body&& body) {
    Entry* e = find(key);
    if (!e) {
      Failure why;
      e = capture(key, stream, hipStreamCaptureModeThreadLocal, body, why);
      if (!e) why.raise();
    }
    HIPCHK(hipGraphLaunch(e->exec, stream));
  }
};

}  // namespace amgx
