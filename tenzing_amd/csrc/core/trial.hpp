// Collective agreement on local failures, the verified trial the transport preflights run, and
// the layout of the blobs the IPC transports allgather. Host only (no HIP): the unit suite links
// it and runs the trial on ranks as threads.
//
// Reference: none (the reference's transports are MPI calls that either work or abort the job).
#pragma once

#include "core/ctrl.hpp"
#include "core/util.hpp"

#include <algorithm>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

namespace tz {

/// `name` is in the comma list of env TZ_FAIL_TRANSPORTS (tests: simulated failures)
inline bool fail_simulated(const std::string &name) {
  const char *f = std::getenv("TZ_FAIL_TRANSPORTS");
  return f && ("," + std::string(f) + ",").find("," + name + ",") != std::string::npos;
}

/// One allreduce_max: "" when `why` is empty on every rank, else `why`, or `elsewhere` on the
/// ranks that passed locally. Every rank must call it, whatever failed locally.
inline std::string agree(Ctrl &ctrl, std::string why, const char *elsewhere = "failed on another rank") {
  double bad = why.empty() ? 0.0 : 1.0;
  ctrl.allreduce_max(&bad, 1);
  if (bad == 0.0) return "";
  return why.empty() ? std::string(elsewhere) : why;
}

/// A verified trial of a transport: `exchange` runs it (and synchronizes the device), `verify`
/// returns what is wrong with the result ("" = nothing). Returns "" when every rank passed, else
/// this rank's reason ("<name>: ..."), or "failed on another rank". TZ_FAIL_TRANSPORTS naming
/// `name` fails a trial that passed (the failure branches' tests).
///
/// The invariant: every call makes exactly one barrier and then one allreduce_max, on every rank,
/// whatever throws or fails locally. A rank whose exchange threw skips only its own verify. The
/// barrier is not optional: peers may still be writing into this rank's memory until they have
/// synchronized too.
inline std::string agreed_trial(Ctrl &ctrl, const std::string &name, const std::function<void()> &exchange,
                                const std::function<std::string()> &verify) {
  std::string why;
  try {
    exchange();
  } catch (const std::exception &e) {
    why = name + ": " + e.what();
  }
  ctrl.barrier();
  if (why.empty()) {
    try {
      why = verify();
      if (why.empty() && fail_simulated(name)) why = name + ": simulated failure (TZ_FAIL_TRANSPORTS)";
    } catch (const std::exception &e) {
      why = name + " check: " + e.what();
    }
  }
  return agree(ctrl, std::move(why));
}

/// What a rank exports for its peers to map: [node identity][handles, `H` bytes each][payload].
/// A handle is only meaningful on the node that exported it, and an all-zero one stands for
/// "nothing exported in this slot".
namespace ipc_blob {
inline std::string pack(const std::string &node, const std::vector<std::string> &handles,
                        const std::string &payload = "") {
  std::string b = node;
  for (const std::string &h : handles) b += h;
  return b + payload;
}
/// handle `slot` of a peer's blob, as seen from `node`: long enough, same node, not all-zero
inline std::string handle(const std::string &blob, const std::string &node, size_t H, size_t slot) {
  TZ_CHECK(blob.size() >= node.size() + (slot + 1) * H, "a peer exported no IPC handles");
  TZ_CHECK(blob.compare(0, node.size(), node) == 0, "a peer runs on another node");
  const std::string h = blob.substr(node.size() + slot * H, H);
  TZ_CHECK(std::any_of(h.begin(), h.end(), [](char c) { return c != 0; }),
           "a peer exported no IPC handle in slot " << slot);
  return h;
}
/// the bytes behind `nslots` handles
inline std::string payload(const std::string &blob, size_t nodeBytes, size_t H, size_t nslots) {
  TZ_CHECK(blob.size() >= nodeBytes + nslots * H, "a peer exported no IPC handles");
  return blob.substr(nodeBytes + nslots * H);
}
} // namespace ipc_blob

} // namespace tz
