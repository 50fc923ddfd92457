// Halo workload, relay routing on the 2x2x2 rank grid: a share of every face goes through the
// corner peer (first hop over the corner link, second over an edge link) while the rest goes
// direct; the face split and the split direct put are shared with host split.
#include "halo_internal.hpp"

namespace tz {

// ---------------------------------------------------------------- relay routing (2x2x2)
//
// Per iteration, for every face direction i (counters: see kSlotSets):
//   sender r:      relay_put_direct  share A -> nbr(i)'s receive buffer, arrival slot i
//                  relay_put_corner  share B -> corner c = r+e's relay buffer i, c's slot 2nd+i
//                                    (after c's relay credit, my slot 3nd+i)
//   forwarder c:   relay_forward     wait slot 2nd+i and the final receiver's forward credit
//                                    (slot 5nd+i), copy B behind A in R = c-e+d_i's buffer,
//                                    signal R's slot 4nd+i, return r's relay credit
//   receiver R:    relay_wait        slots i and 4nd+i
//                  relay_unpack      A and B sub-boxes, credits to nbr(-i) and the forwarder
// Puts depend on nothing of the current iteration, forwards only on puts, waits on both, so
// any schedule that issues a rank's forward after its corner put cannot deadlock.

std::vector<int> HaloExchange::relay_faces() const {
  std::vector<int> v;
  for (int i : group_dirs(1))
    if (ipc_[i]) v.push_back(i);
  return v;
}

unsigned long long *HaloExchange::peer_slot(int rank, int set, int i) const {
  TZ_CHECK(rank >= 0 && size_t(rank) < peerFlags_.size() && peerFlags_[size_t(rank)],
           "rank " << rank << " is not IPC-mapped");
  return static_cast<unsigned long long *>(peerFlags_[size_t(rank)]) + size_t(set) * ndirs() + i;
}

void HaloExchange::split_box(const kern::BoxDesc &b, double frac, kern::BoxDesc &A,
                             kern::BoxDesc &B) const {
  // largest of (n1, n2, n3), the slower dimension on ties
  int32_t n[3] = {b.n1, b.n2, b.n3};
  const int64_t st[3] = {b.s1, b.s2, b.s3};
  int k = 2;
  for (int j = 1; j >= 0; --j)
    if (n[j] > n[k]) k = j;
  TZ_CHECK(n[k] >= 2, "box too small to split for relay routing");
  const int32_t nb = std::min<int32_t>(n[k] - 1, std::max<int32_t>(1, int32_t(std::lround(frac * n[k]))));
  A = b;
  B = b;
  int32_t *na[3] = {&A.n1, &A.n2, &A.n3};
  int32_t *nbp[3] = {&B.n1, &B.n2, &B.n3};
  *na[k] = n[k] - nb;
  *nbp[k] = nb;
  B.grid_off = b.grid_off + int64_t(n[k] - nb) * st[k];
  // B starts on a 128-B boundary behind A in the receive buffer (the buffers have the slack)
  const size_t aElems = size_t(A.len) * A.n1 * A.n2 * A.n3;
  B.buf = b.buf ? b.buf + round_up(int64_t(aElems), 16) : nullptr;
}

void HaloExchange::relay_put_direct(const std::vector<int> &dirs, double frac, void *stream) const {
  TZ_CHECK(ready() && relayReady_, "relay routing not set up");
  split_put_direct(dirs, frac, stream);
}

void HaloExchange::split_put_direct(const std::vector<int> &dirs, double frac, void *stream) const {
  TZ_CHECK(ready() && ipcReady_ && !ipcGrid_, "ipc buffers mode not set up");
  TZ_CHECK(!dirs.empty() && dirs.size() <= size_t(kern::kMaxBoxes), "bad split put group");
  const std::vector<int> faces = relay_faces();
  std::vector<kern::BoxDesc> bs;
  kern::MoveSignal sig;
  sig.done = done_.as<unsigned int>() + size_t(dirs.front()) * kern::kMaxBoxes;
  kern::ipc_wait(flags_.as<const unsigned long long>() + ndirs(), sent_.as<unsigned long long>(),
                 dirs.data(), int(dirs.size()), err_.as<int>(), ipcTimeoutS_, stream, /*lag=*/1);
  for (size_t k = 0; k < dirs.size(); ++k) {
    const int i = dirs[k];
    TZ_CHECK(i >= 0 && i < ndirs() && ipc_[i], "direction " << i << " is not an ipc put");
    kern::BoxDesc b = make_box(a_, dirs_[i], false, xoff_, sy_, sz_, sq_);
    b.buf = static_cast<double *>(peerRecv_[size_t(i)]);
    if (std::find(faces.begin(), faces.end(), i) != faces.end()) {
      kern::BoxDesc B;
      split_box(kern::BoxDesc(b), frac, b, B);
    }
    bs.push_back(b);
    sig.flag[k] = peer_slot(nbr_[i], 0, i);
  }
  kern::box_pack_many_signal(grid(), bs.data(), int(bs.size()), sig, stream);
}

void HaloExchange::relay_put_corner(const std::vector<int> &faces, double frac, void *stream) const {
  TZ_CHECK(ready() && relayReady_, "relay routing not set up");
  TZ_CHECK(!faces.empty() && faces.size() <= size_t(kern::kMaxBoxes), "bad relay face group");
  const int nd = ndirs();
  unsigned long long *book = relayBook_.as<unsigned long long>();
  // the corner peer must have forwarded my previous shares out of its relay buffers
  kern::ipc_wait(flags_.as<const unsigned long long>() + 3 * nd, book + nd, faces.data(),
                 int(faces.size()), err_.as<int>(), ipcTimeoutS_, stream, /*lag=*/1);
  std::vector<kern::BoxDesc> bs;
  kern::MoveSignal sig;
  sig.done = done_.as<unsigned int>() + size_t(nd + faces.front()) * kern::kMaxBoxes;
  for (size_t k = 0; k < faces.size(); ++k) {
    const int i = faces[k];
    TZ_CHECK(peerRelay_.size() > size_t(i) && peerRelay_[size_t(i)], "direction " << i << " is not relayed");
    kern::BoxDesc A, B;
    split_box(make_box(a_, dirs_[i], false, xoff_, sy_, sz_, sq_), frac, A, B);
    B.buf = static_cast<double *>(peerRelay_[size_t(i)]); // dense at the relay buffer's start
    bs.push_back(B);
    sig.flag[k] = peer_slot(corner_, 2, i);
  }
  kern::box_pack_many_signal(grid(), bs.data(), int(bs.size()), sig, stream);
}

void HaloExchange::relay_forward(const std::vector<int> &faces, double frac, void *stream,
                                 bool sdma) const {
  TZ_CHECK(ready() && relayReady_, "relay routing not set up");
  TZ_CHECK(!faces.empty() && faces.size() <= size_t(kern::kMaxBoxes), "bad relay face group");
  const int nd = ndirs();
  unsigned long long *book = relayBook_.as<unsigned long long>();
  const unsigned long long *fl = flags_.as<const unsigned long long>();
  // the origin's shares arrived in my relay buffers; the final receivers consumed what I
  // forwarded last time
  kern::ipc_wait(fl + 2 * nd, book, faces.data(), int(faces.size()), err_.as<int>(), ipcTimeoutS_,
                 stream, /*lag=*/0);
  kern::ipc_wait(fl + 5 * nd, book + 3 * nd, faces.data(), int(faces.size()), err_.as<int>(),
                 ipcTimeoutS_, stream, /*lag=*/1);
  std::vector<kern::MoveDesc> ms;
  std::vector<unsigned long long *> credits;
  kern::MoveSignal sig;
  sig.done = done_.as<unsigned int>() + size_t(2 * nd + faces.front()) * kern::kMaxBoxes;
  for (size_t k = 0; k < faces.size(); ++k) {
    const int i = faces[k];
    TZ_CHECK(peerFwdRecv_.size() > size_t(i) && peerFwdRecv_[size_t(i)] && relayBuf_[i].get(),
             "direction " << i << " is not forwarded");
    // the share has the shape of my own box i (the origin's box i); it goes behind the direct
    // share in the final receiver's buffer of ghost side -d_i: one contiguous run
    kern::BoxDesc b = make_box(a_, dirs_[i], false, xoff_, sy_, sz_, sq_), A, B;
    b.buf = nullptr;
    split_box(b, frac, A, B);
    const int64_t aElems = int64_t(A.len) * A.n1 * A.n2 * A.n3;
    const int64_t bElems = int64_t(B.len) * B.n1 * B.n2 * B.n3;
    TZ_CHECK(bElems < (int64_t(1) << 31), "relayed share too large");
    kern::MoveDesc m;
    m.src = relayBuf_[i].as<double>();
    m.dst = static_cast<double *>(peerFwdRecv_[size_t(i)]);
    m.src_off = 0;
    m.dst_off = round_up(aElems, 16);
    m.len = int32_t(bElems);
    m.n1 = m.n2 = m.n3 = 1;
    ms.push_back(m);
    sig.flag[k] = peer_slot(fwdTo_[i], 4, i);
    credits.push_back(peer_slot(relayOrigin_, 3, i));
  }
  if (!sdma) {
    kern::box_move_many_signal(ms.data(), int(ms.size()), sig, stream);
  } else {
    std::vector<Copy> cs;
    for (const kern::MoveDesc &m : ms) cs.push_back({m.dst + m.dst_off, m.src, size_t(m.len) * sizeof(double)});
    engine_copies(cs, stream);
    // arrivals are published after the copies (stream order), like copy-engine puts
    for (size_t k = 0; k < faces.size(); ++k) credits.push_back(sig.flag[k]);
  }
  // the relay buffers are free again: the origin may put its next shares
  kern::ipc_signal(credits.data(), int(credits.size()), stream);
}

void HaloExchange::relay_wait(const std::vector<int> &dirs, const std::vector<int> &faces,
                              void *stream) const {
  TZ_CHECK(ready() && relayReady_, "relay routing not set up");
  const unsigned long long *fl = flags_.as<const unsigned long long>();
  kern::ipc_wait(fl, expected_.as<unsigned long long>(), dirs.data(), int(dirs.size()), err_.as<int>(),
                 ipcTimeoutS_, stream, /*lag=*/0);
  kern::ipc_wait(fl + 4 * ndirs(), relayBook_.as<unsigned long long>() + 2 * ndirs(), faces.data(),
                 int(faces.size()), err_.as<int>(), ipcTimeoutS_, stream, /*lag=*/0);
}

void HaloExchange::relay_unpack(const std::vector<int> &dirs, const std::vector<int> &faces,
                                double frac, void *stream) const {
  TZ_CHECK(ready() && relayReady_, "relay routing not set up");
  std::vector<kern::BoxDesc> bs;
  std::vector<unsigned long long *> credits = credit_ptrs(dirs);
  for (int i : dirs) {
    check_pipelined(i);
    const kern::BoxDesc u = unpack_box(opp_[i]); // buf = my receive buffer of ghost side -d_i
    if (std::find(faces.begin(), faces.end(), i) == faces.end()) {
      bs.push_back(u);
      continue;
    }
    kern::BoxDesc A, B;
    split_box(u, frac, A, B);
    bs.push_back(A);
    bs.push_back(B);
    credits.push_back(peer_slot(fwdFrom_[i], 5, i));
  }
  for (size_t k = 0; k < bs.size(); k += kern::kMaxBoxes)
    kern::box_copy_many(grid(), bs.data() + k, int(std::min<size_t>(kern::kMaxBoxes, bs.size() - k)),
                        true, stream);
  kern::ipc_signal(credits.data(), int(credits.size()), stream);
}

void HaloExchange::relay_preflight(Ctrl *ctrl) {
  // one verified relayed exchange per offered share (a new value generation each) before the
  // search may use relay routing; a failure turns it off on every rank (ipc puts without relay
  // remain)
  const std::vector<int> faces = relay_faces();
  std::string why;
  int gen = 0;
  for (double f : a_.relay_fracs) {
    why = preflight_trial(
        ctrl, "relay", 1 + gen++ % 3,
        [&](const DirLists &d) {
          relay_put_direct(d.remote, f, nullptr);
          relay_put_corner(faces, f, nullptr);
          relay_forward(faces, f, nullptr);
          relay_wait(d.remote, faces, nullptr);
          relay_unpack(d.remote, faces, f, nullptr);
        },
        " (share " + std::to_string(f) + ")");
    if (!why.empty()) break;
  }
  if (!why.empty()) {
    relayReady_ = false;
    relayWhy_ = why;
    TZ_LOG(Warn, "relay routing disabled: " << why);
    reset_ipc_counters(ctrl);
    TZ_CHECK(a_.relay != "force", "relay routing forced but " << why);
  }
  init_grid();
}

} // namespace tz
