// Native unit tests of the core (no GPU, no Python). Mirrors the reference's in-source doctest
// cases (src/operation.cpp:87-101 "[cpu] op eq", src/graph.cpp:422-501 graph construction /
// clone / replace / expand, src/sequence.cpp:169-176) and test/test_noop_graph.cpp,
// test/test_gpu_graph.cu (decision generation under 2 streams and stream-swap equivalence),
// plus synchronizer race-freedom, redundant-sync removal, serdes round trips and solvers.
// Run: tenzing_amd/bin/tz-unit [filter]
#include "core/benchmark.hpp"
#include "core/ctrl.hpp"
#include "core/deadline_claim.hpp"
#include "core/health.hpp"
#include "core/solve.hpp"
#include "core/trial.hpp"

#include <arpa/inet.h>
#include <netinet/in.h>
#include <sys/select.h>
#include <sys/socket.h>
#include <unistd.h>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <future>
#include <iostream>
#include <thread>
#include <random>
#include <set>
#include <string>
#include <vector>

using namespace tz;

static int g_fail = 0, g_checks = 0;
#define CHECK(c)                                                                                   \
  do {                                                                                             \
    ++g_checks;                                                                                    \
    if (!(c)) {                                                                                    \
      ++g_fail;                                                                                    \
      std::fprintf(stderr, "  CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);                  \
    }                                                                                              \
  } while (0)

struct TestCase {
  const char *name;
  std::function<void()> fn;
};
static std::vector<TestCase> &cases() {
  static std::vector<TestCase> c;
  return c;
}
struct Reg {
  Reg(const char *n, std::function<void()> f) { cases().push_back({n, std::move(f)}); }
};
#define TEST(name)                                                                                 \
  static void name();                                                                              \
  static Reg reg_##name(#name, name);                                                              \
  static void name()

static std::shared_ptr<Graph> diamond(double a = 10, double b = 20, double c = 30, double d = 5) {
  auto g = std::make_shared<Graph>();
  auto k1 = std::make_shared<SimGpuOp>("k1", a);
  auto k2 = std::make_shared<SimGpuOp>("k2", b);
  auto k3 = std::make_shared<SimGpuOp>("k3", c);
  auto k4 = std::make_shared<SimGpuOp>("k4", d);
  g->start_then(k1);
  g->then(k1, k2);
  g->then(k1, k3);
  g->then(k2, k4);
  g->then(k3, k4);
  g->then_finish(k4);
  return g;
}

TEST(json_roundtrip) {
  Json j = Json::parse(R"({"b":[1,2.5,"x\n",true,null],"a":{"k":-3}})");
  CHECK(j.at("a").at("k").as_int() == -3);
  CHECK(j.at("b").at(1).as_double() == 2.5);
  CHECK(j.dump() == R"({"a":{"k":-3},"b":[1,2.5,"x\n",true,null]})");
  CHECK(Json::parse(j.dump()) == j);
}

TEST(op_eq) {
  NoOp a("a"), a2("a"), b("b");
  CHECK(a.eq(a2));
  CHECK(!a.eq(b));
  EventRecord r1(0, 1, "x"), r2(0, 1, "y"), r3(1, 1);
  CHECK(r1.eq(r2));
  CHECK(!r1.eq(r3));
  CHECK(r1.json().dump() == R"({"event":0,"kind":"CudaEventRecord","name":"x","stream":1})");
}

TEST(graph_build_clone_replace_expand) {
  auto g = diamond();
  g->normalize();
  CHECK(g->size() == 6);
  CHECK(g->num_edges() == 6);
  CHECK(g->succs(Graph::kStart).size() == 1);
  auto topo = g->topo_order();
  CHECK(topo.front() == Graph::kStart && topo.back() == Graph::kFinish);
  const int k2 = g->find("k2");
  auto g2 = g->clone_but_replace(k2, std::make_shared<SimGpuOp>("k2b", 1));
  CHECK(g2->find("k2") < 0 && g2->find("k2b") == k2);
  CHECK(g->find("k2") == k2);
  // expand a compound op into the outer graph
  auto outer = std::make_shared<Graph>();
  auto sub = std::make_shared<Graph>();
  auto x = std::make_shared<NoOp>("x"), y = std::make_shared<NoOp>("y");
  sub->start_then(x);
  sub->then(x, y);
  sub->then_finish(y);
  auto c = std::make_shared<StaticCompoundOp>("c", sub);
  auto pre = std::make_shared<NoOp>("pre"), post = std::make_shared<NoOp>("post");
  outer->start_then(pre);
  outer->then(pre, c);
  outer->then(c, post);
  outer->then_finish(post);
  auto e = outer->clone_but_expand(outer->find("c"), *sub);
  CHECK(e->find("c") < 0);
  CHECK(e->size() == 6);
  const int ix = e->find("x"), iy = e->find("y");
  CHECK(e->preds(ix).size() == 1 && e->op(e->preds(ix)[0])->name() == "pre");
  CHECK(e->succs(iy).size() == 1 && e->op(e->succs(iy)[0])->name() == "post");
}

TEST(noop_graph_decisions) {
  // reference test/test_noop_graph.cpp:10-42
  auto g = std::make_shared<Graph>();
  auto op1 = std::make_shared<NoOp>("op1");
  g->start_then(op1);
  g->then_finish(op1);
  State s(g, Platform::make_n_streams(2));
  CHECK(s.sequence().size() == 1);
  auto ds = s.get_decisions();
  int count = 0;
  for (auto &d : ds) count += d.kind == Decision::Kind::Execute && d.op->name() == "op1";
  CHECK(count == 1);
  for (auto &d : ds) CHECK(s.apply(d).sequence().size() == 2);
}

TEST(gpu_graph_decisions_and_equivalence) {
  // reference test/test_gpu_graph.cu:41-118
  auto g = std::make_shared<Graph>();
  auto k1 = std::make_shared<SimGpuOp>("kernel1", 1), k2 = std::make_shared<SimGpuOp>("kernel2", 1),
       k3 = std::make_shared<SimGpuOp>("kernel3", 1);
  g->start_then(k1);
  g->then(k1, k2);
  g->then(k1, k3);
  g->then_finish(k2);
  g->then_finish(k3);
  Platform nonsym = Platform::make_n_streams(2);
  nonsym.symmetric_streams = false;
  State s0(g, nonsym);
  auto ds = s0.get_decisions();
  int a0 = 0, a1 = 0;
  for (auto &d : ds) {
    a0 += d.kind == Decision::Kind::Assign && d.stream == 0;
    a1 += d.kind == Decision::Kind::Assign && d.stream == 1;
  }
  CHECK(a0 == 1 && a1 == 1);
  State sa = s0.apply(ds[0]), sb = s0.apply(ds[1]);
  CHECK(sa.sequence().size() == 1);
  // binding kernel1 to stream 0 or 1 is equivalent under a stream bijection
  State sa2(g, Platform::make_n_streams(2)), sb2(g, Platform::make_n_streams(2));
  Decision d0, d1;
  d0.kind = d1.kind = Decision::Kind::Assign;
  d0.node = d1.node = sa2.graph().find("kernel1");
  d0.stream = 0;
  d1.stream = 1;
  CHECK(equivalent(sa2.apply(d0), sb2.apply(d1)));
  // symmetric platform offers only one fresh stream initially
  State s1(g, Platform::make_n_streams(2));
  CHECK(s1.get_decisions().size() == 1);
  // after binding, kernel1 is executable
  auto ds2 = sa.get_decisions();
  CHECK(ds2.size() == 1 && ds2[0].kind == Decision::Kind::Execute && ds2[0].op->name() == "kernel1");
}

TEST(synchronizer_inserts_syncs) {
  auto g = diamond();
  Platform p = Platform::make_n_streams(2);
  State s(g, p);
  auto exec = [&](const std::string &kind, int stream) {
    for (auto &d : s.get_decisions()) {
      if (kind == "assign" && d.kind == Decision::Kind::Assign && d.stream == stream) {
        s.apply_inplace(d);
        return true;
      }
      if (kind == "exec" && d.kind == Decision::Kind::Execute) {
        s.apply_inplace(d);
        return true;
      }
    }
    return false;
  };
  CHECK(exec("assign", 0)); // k1 -> s0
  CHECK(exec("exec", 0));   // k1
  // k2, k3 frontier: assign k2 -> s1 (second stream)
  bool ok = false;
  for (auto &d : s.get_decisions())
    if (d.kind == Decision::Kind::Assign && s.graph().op(d.node)->name() == "k2" && d.stream == 1) {
      s.apply_inplace(d);
      ok = true;
      break;
    }
  CHECK(ok);
  // k2 on s1 depends on k1 on s0 -> decisions must contain a CER on stream 0, not k2 itself
  bool sawCer = false, sawK2 = false;
  for (auto &d : s.get_decisions()) {
    if (d.kind != Decision::Kind::Execute) continue;
    if (d.op->kind() == "CudaEventRecord" && static_cast<const SyncOp &>(*d.op).stream() == 0) sawCer = true;
    if (d.op->name() == "k2") sawK2 = true;
  }
  CHECK(sawCer && !sawK2);
}

TEST(every_rollout_is_race_free) {
  std::mt19937_64 rng(7);
  for (int streams = 1; streams <= 3; ++streams) {
    auto g = diamond();
    for (int t = 0; t < 200; ++t) {
      State s(g, Platform::make_n_streams(streams));
      Sequence seq = random_rollout(s, rng);
      // final graph == normalized g here (no compound/choice)
      Graph ng = *g;
      ng.normalize();
      CHECK(verify(seq, ng, streams).empty());
      Sequence r = seq;
      remove_redundant_syncs(r, ng, streams);
      CHECK(verify(r, ng, streams).empty());
      CHECK(r.count_sync_ops() <= seq.count_sync_ops());
    }
  }
}

TEST(verify_detects_race) {
  auto g = diamond();
  Graph ng = *g;
  ng.normalize();
  auto k = [&](const char *n) { return std::static_pointer_cast<const GpuOp>(ng.op(ng.find(n))); };
  Sequence s;
  s.push_back(std::make_shared<Start>());
  s.push_back(std::make_shared<BoundGpuOp>(k("k1"), 0));
  s.push_back(std::make_shared<BoundGpuOp>(k("k2"), 1)); // races with k1 (no event)
  s.push_back(std::make_shared<BoundGpuOp>(k("k3"), 0));
  s.push_back(std::make_shared<BoundGpuOp>(k("k4"), 0));
  s.push_back(std::make_shared<Finish>());
  auto v = verify(s, ng, 2);
  CHECK(v.size() >= 2); // k2 after k1, k4 after k2, Finish after k4
  // fixed version
  Sequence f;
  f.push_back(std::make_shared<Start>());
  f.push_back(std::make_shared<BoundGpuOp>(k("k1"), 0));
  f.push_back(std::make_shared<EventRecord>(0, 0));
  f.push_back(std::make_shared<StreamWaitEvent>(1, 0));
  f.push_back(std::make_shared<BoundGpuOp>(k("k2"), 1));
  f.push_back(std::make_shared<BoundGpuOp>(k("k3"), 0));
  f.push_back(std::make_shared<StreamWait>(0, 1));
  f.push_back(std::make_shared<BoundGpuOp>(k("k4"), 0));
  f.push_back(std::make_shared<StreamSync>(0));
  f.push_back(std::make_shared<Finish>());
  CHECK(verify(f, ng, 2).empty());
}

TEST(serdes_roundtrip) {
  auto g = diamond();
  std::mt19937_64 rng(3);
  Sequence seq = random_rollout(State(g, Platform::make_n_streams(2)), rng);
  OpIndex idx(*g);
  Sequence back = idx.sequence_from_json(Json::parse(seq.json(true).dump()));
  CHECK(back.size() == seq.size());
  CHECK(back.canonical_key() == seq.canonical_key());
  for (size_t i = 0; i < seq.size(); ++i) CHECK(back[i]->eq(*seq[i]));
}

TEST(equivalence_under_relabel) {
  auto g = diamond();
  Graph ng = *g;
  ng.normalize();
  auto k = [&](const char *n) { return std::static_pointer_cast<const GpuOp>(ng.op(ng.find(n))); };
  auto build = [&](int s0, int s1, int e) {
    Sequence s;
    s.push_back(std::make_shared<Start>());
    s.push_back(std::make_shared<BoundGpuOp>(k("k1"), s0));
    s.push_back(std::make_shared<EventRecord>(e, s0));
    s.push_back(std::make_shared<StreamWaitEvent>(s1, e));
    s.push_back(std::make_shared<BoundGpuOp>(k("k2"), s1));
    return s;
  };
  CHECK(equivalent(build(0, 1, 0), build(1, 0, 3)));
  CHECK(!equivalent(build(0, 1, 0), build(0, 0, 0)));
}

TEST(dfs_enumerates_and_dedups) {
  auto g = diamond();
  for (int streams = 1; streams <= 2; ++streams) {
    auto seqs = get_all_sequences(*g, Platform::make_n_streams(streams), -1);
    CHECK(!seqs.empty());
    Graph ng = *g;
    ng.normalize();
    std::set<std::string> keys;
    for (auto &s : seqs) {
      CHECK(verify(s, ng, streams).empty());
      keys.insert(s.canonical_key());
    }
    CHECK(keys.size() == seqs.size());
    if (streams == 1) CHECK(seqs.size() == 2); // k2/k3 order
  }
}

TEST(sim_prefers_overlap) {
  auto g = diamond(10, 100, 100, 10);
  SimParams p;
  p.launch_us = 1;
  SimBenchmarker sb(2, p);
  BenchOpts bo;
  bo.n_iters = 3;
  auto seqs = get_all_sequences(*g, Platform::make_n_streams(2), -1);
  double best = 1e9, worst = 0;
  for (auto &s : seqs) {
    double t = sb.benchmark(s, bo).pct10;
    best = std::min(best, t);
    worst = std::max(worst, t);
  }
  CHECK(best < 180e-6);  // k2 || k3 on two streams
  CHECK(worst > 200e-6); // serialized
}

TEST(sim_graph_replay_costs) {
  // SimParams::graph on a diamond 10 -> (100 || 100) -> 10: on one stream four ops in a row pay
  // a 1-us gap each; the best two-stream schedule pays one cross-stream wait on each side of
  // the overlap (5.5 us after the op it waits on) and the end-of-iteration join of two streams
  auto g = diamond(10, 100, 100, 10);
  SimParams p;
  p.graph = true;
  for (auto &s : get_all_sequences(*g, Platform::make_n_streams(1), -1)) {
    SimExecutor ex(1, p);
    CHECK(std::abs(ex.run_once(s) - (220.0 + 4 * p.graph_gap_us)) < 1e-6);
  }
  double best = 1e9;
  auto seqs = get_all_sequences(*g, Platform::make_n_streams(2), -1);
  for (auto &s : seqs) {
    SimExecutor ex(2, p);
    best = std::min(best, ex.run_once(s));
  }
  // k1 [0,10] | k3 on the other stream from 10 + 5.5, k2 after k1 + gap | k4 on k3's stream at
  // k2's end + 5.5 | + the join
  CHECK(std::abs(best - (10 + p.graph_join_us + 100 + p.graph_gap_us + 10 + p.graph_join_us)) < 1e-6);
}

TEST(mcts_finds_good_schedule) {
  auto g = diamond(10, 100, 100, 10);
  SimParams p;
  p.launch_us = 1;
  SelfCtrl ctrl;
  for (const auto &strat : strategy_names()) {
    SimBenchmarker sb(2, p);
    MctsOpts o;
    o.n_iters = 60;
    o.strategy = strat;
    o.seed = 5;
    o.bench.n_iters = 3;
    SearchResult r = mcts_explore(*g, Platform::make_n_streams(2), sb, ctrl, o);
    CHECK(!r.sims.empty());
    CHECK(r.best() >= 0);
    if (strat == "FastMin") CHECK(r.sims[r.best()].res.pct10 < 180e-6);
  }
}

TEST(mcts_large_tree_stops) {
  // reference Stop::Reason::large_tree (tenzing-mcts mcts.hpp:131)
  auto g = diamond(10, 100, 100, 10);
  SimBenchmarker sb(4, SimParams());
  SelfCtrl ctrl;
  MctsOpts o;
  o.n_iters = 0;
  o.max_tree_nodes = 50;
  o.bench.n_iters = 2;
  SearchResult r = mcts_explore(*g, Platform::make_n_streams(4), sb, ctrl, o);
  CHECK(r.stop_reason == "large_tree");
  CHECK(r.tree_size >= 50);
  CHECK(!r.sims.empty());
}

TEST(mcts_seed_schedules_join_the_tree) {
  auto g = diamond(10, 100, 100, 10);
  auto gp = std::make_shared<Graph>(*g);
  gp->normalize();
  std::mt19937_64 rng(7);
  MctsOpts o;
  o.n_iters = 2;
  o.bench.n_iters = 2;
  std::set<std::string> keys;
  for (int k = 0; k < 10; ++k) {
    Sequence s = random_rollout(State(gp, Platform::make_n_streams(3)), rng);
    remove_redundant_syncs(s, *resolve_graph(*gp, s), 3);
    keys.insert(s.canonical_key());
    o.seed_schedules.push_back(s);
  }
  SimBenchmarker sb(3, SimParams());
  SelfCtrl ctrl;
  SearchResult r = mcts_explore(*g, Platform::make_n_streams(3), sb, ctrl, o);
  size_t seeded = 0;
  for (const auto &s : r.sims) seeded += s.seeded;
  CHECK(seeded == o.seed_schedules.size());
  CHECK(r.counters.counts.count("SEED_IN_TREE") && r.counters.counts.at("SEED_IN_TREE") >= keys.size());
}

TEST(mcts_full_tree_stops) {
  auto g = std::make_shared<Graph>();
  auto a = std::make_shared<NoOp>("a"), b = std::make_shared<NoOp>("b");
  g->start_then(a);
  g->start_then(b);
  g->then_finish(a);
  g->then_finish(b);
  SimBenchmarker sb(1, SimParams());
  SelfCtrl ctrl;
  MctsOpts o;
  o.n_iters = 100;
  o.bench.n_iters = 2;
  SearchResult r = mcts_explore(*g, Platform::make_n_streams(1), sb, ctrl, o);
  CHECK(r.stop_reason == "full_tree");
  CHECK(r.sims.size() <= 4);
}

TEST(csv_benchmarker_replay) {
  auto g = diamond();
  SimBenchmarker sb(2, SimParams());
  SelfCtrl ctrl;
  DfsOpts o;
  o.bench.n_iters = 2;
  SearchResult r = dfs_explore(*g, Platform::make_n_streams(2), sb, ctrl, o);
  const std::string path = "/tmp/tz_unit_replay.csv";
  {
    std::ofstream f(path);
    r.dump_csv(f);
  }
  CsvBenchmarker cb(path, *g);
  CHECK(cb.size() == r.sims.size());
  for (auto &s : r.sims) CHECK(std::abs(cb.benchmark(s.seq, o.bench).pct10 - s.res.pct10) < 1e-12);
  std::remove(path.c_str());
}

TEST(choice_and_compound_in_search) {
  auto sub = std::make_shared<Graph>();
  auto x = std::make_shared<SimGpuOp>("x", 5);
  auto fast = std::make_shared<SimGpuOp>("y_fast", 5), slow = std::make_shared<SimGpuOp>("y_slow", 50);
  auto ch = std::make_shared<StaticChoiceOp>("y", std::vector<OpPtr>{slow, fast});
  sub->start_then(x);
  sub->then(x, ch);
  sub->then_finish(ch);
  auto c = std::make_shared<StaticCompoundOp>("comp", sub);
  auto g = std::make_shared<Graph>();
  g->start_then(c);
  g->then_finish(c);
  auto seqs = get_all_sequences(*g, Platform::make_n_streams(2), -1);
  bool sawFast = false, sawSlow = false;
  for (auto &s : seqs)
    for (auto &e : s.entries) {
      sawFast |= e.op->name() == "y_fast";
      sawSlow |= e.op->name() == "y_slow";
    }
  CHECK(sawFast && sawSlow);
  SimBenchmarker sb(2, SimParams());
  SelfCtrl ctrl;
  MctsOpts o;
  o.n_iters = 40;
  o.bench.n_iters = 2;
  SearchResult r = mcts_explore(*g, Platform::make_n_streams(2), sb, ctrl, o);
  bool bestFast = false;
  for (auto &e : r.sims[r.best()].seq.entries) bestFast |= e.op->name() == "y_fast";
  CHECK(bestFast);
  // schedules deserialize against the original (unexpanded) graph
  OpIndex idx(*g);
  Sequence back = idx.sequence_from_json(Json::parse(r.sims[0].seq.json().dump()));
  CHECK(back.canonical_key() == r.sims[0].seq.canonical_key());
  // ... and verify against the graph they executed (choice resolved, compound expanded)
  for (const auto &sim : r.sims) {
    Sequence loaded = idx.sequence_from_json(sim.seq.json(true));
    GraphPtr fg = resolve_graph(*g, loaded);
    CHECK(fg->find("comp") < 0 && fg->find("y") < 0 && fg->find("x") >= 0);
    CHECK(verify(loaded, *fg, 2).empty());
  }
}

TEST(mcts_checkpoint_resume) {
  auto g = diamond(10, 100, 100, 10);
  SelfCtrl ctrl;
  SimBenchmarker sb(2, SimParams());
  MctsOpts o;
  o.n_iters = 20;
  o.bench.n_iters = 2;
  o.checkpoint_path = "/tmp/tz_unit_ck.json";
  SearchResult r1 = mcts_explore(*g, Platform::make_n_streams(2), sb, ctrl, o);
  MctsOpts o2 = o;
  o2.resume_path = o.checkpoint_path;
  o2.checkpoint_path = "";
  o2.n_iters = 30;
  SearchResult r2 = mcts_explore(*g, Platform::make_n_streams(2), sb, ctrl, o2);
  CHECK(r2.sims.size() >= r1.sims.size());
  std::remove(o.checkpoint_path.c_str());
}

TEST(tcp_ctrl_rendezvous_skips_a_foreign_listener) {
  // the torch-free bootstrap: rank 0 listens on the first free of several candidate ports (the
  // first is held by a "foreign" listener that accepts and never answers), the other ranks try
  // the candidates and take the one that acknowledges their handshake; then one collective
  int probe = ::socket(AF_INET, SOCK_STREAM, 0);
  sockaddr_in a{};
  a.sin_family = AF_INET;
  a.sin_addr.s_addr = htonl(INADDR_LOOPBACK);
  a.sin_port = 0;
  CHECK(::bind(probe, reinterpret_cast<sockaddr *>(&a), sizeof(a)) == 0);
  socklen_t len = sizeof(a);
  ::getsockname(probe, reinterpret_cast<sockaddr *>(&a), &len);
  const int base = ntohs(a.sin_port);
  CHECK(::listen(probe, 8) == 0); // the foreign listener on the first candidate port
  std::atomic<bool> stop{false};
  std::vector<int> held;
  std::thread foreign([&] {
    while (!stop.load()) {
      fd_set rd;
      FD_ZERO(&rd);
      FD_SET(probe, &rd);
      timeval tv{0, 100000};
      if (::select(probe + 1, &rd, nullptr, nullptr, &tv) > 0) held.push_back(::accept(probe, nullptr, nullptr));
    }
  });
  constexpr int N = 3;
  std::vector<std::string> got(N), err(N);
  auto body = [&](int r) {
    try {
      TcpCtrl c(r, N);
      c.rendezvous("127.0.0.1", base, 60.0, 4);
      std::string s = r == 0 ? "hello" : "";
      c.bcast(s, 0);
      got[r] = s;
    } catch (const std::exception &e) {
      err[r] = e.what();
    }
  };
  std::vector<std::thread> ts;
  for (int r = 0; r < N; ++r) ts.emplace_back(body, r);
  for (auto &t : ts) t.join();
  stop = true;
  foreign.join();
  for (int fd : held)
    if (fd >= 0) ::close(fd);
  ::close(probe);
  for (int r = 0; r < N; ++r) {
    if (!err[r].empty()) std::fprintf(stderr, "  rank %d: %s\n", r, err[r].c_str());
    CHECK(err[r].empty() && got[r] == "hello");
  }
}

TEST(tcp_ctrl_ranks_as_threads) {
  // the control plane (reference MPI_Bcast / MPI_Barrier / MPI_Allreduce call sites) with 4
  // ranks as threads of one process, then a collective MCTS search over it: rank 0 owns the
  // tree, every rank runs every candidate. Under the TSan build this is the data-race check of
  // the control plane and of the solver's collective protocol.
  constexpr int N = 4;
  std::promise<int> portP;
  std::shared_future<int> port = portP.get_future().share();
  struct Out {
    std::string bc;
    double mx = 0, sm = 0;
    std::vector<std::string> ag;
    size_t sims = 0;
    double best = 0;
    std::string err;
  };
  std::vector<Out> out(N);
  auto body = [&](int r) {
    try {
      TcpCtrl c(r, N);
      if (r == 0) portP.set_value(c.listen(0, "127.0.0.1"));
      c.connect("127.0.0.1", port.get(), 30.0);
      c.barrier();
      std::string s = r == 2 ? "from-two" : "";
      c.bcast(s, 2);
      out[r].bc = s;
      double v[2] = {double(r), double(10 * r)};
      c.allreduce_max(v, 2);
      out[r].mx = v[0] + v[1];
      double w = 1.0 + r;
      c.allreduce_sum(&w, 1);
      out[r].sm = w;
      out[r].ag = c.allgather("r" + std::to_string(r));
      auto g = diamond(10, 100, 100, 10);
      SimParams p;
      p.launch_us = 1;
      SimBenchmarker sb(2, p);
      MctsOpts o;
      o.n_iters = 12;
      o.seed = 3;
      o.bench.n_iters = 2;
      SearchResult res = mcts_explore(*g, Platform::make_n_streams(2), sb, c, o);
      out[r].sims = res.sims.size();
      if (r == 0 && res.best() >= 0) out[r].best = res.sims[res.best()].res.pct10;
      c.barrier();
    } catch (const std::exception &e) {
      out[r].err = e.what();
      if (r == 0) {
        try {
          portP.set_value(-1);
        } catch (...) {
        }
      }
    }
  };
  std::vector<std::thread> ts;
  for (int r = 0; r < N; ++r) ts.emplace_back(body, r);
  for (auto &t : ts) t.join();
  for (int r = 0; r < N; ++r) {
    if (!out[r].err.empty()) std::fprintf(stderr, "  rank %d: %s\n", r, out[r].err.c_str());
    CHECK(out[r].err.empty());
    CHECK(out[r].bc == "from-two");
    CHECK(out[r].mx == double(N - 1) + double(10 * (N - 1)));
    CHECK(out[r].sm == double(N * (N + 1) / 2));
    CHECK(out[r].ag.size() == size_t(N));
    for (int q = 0; q < N && q < int(out[r].ag.size()); ++q) CHECK(out[r].ag[q] == "r" + std::to_string(q));
    CHECK(out[r].sims == (r == 0 ? size_t(12) : size_t(0)));
  }
  CHECK(out[0].best > 0);
}

/// run `body(rank, ctrl)` on N ranks as threads of this process over a loopback TcpCtrl; returns
/// each rank's exception message ("" = none)
static std::vector<std::string> tcp_ranks(int N, const std::function<void(int, TcpCtrl &)> &body) {
  std::promise<int> portP;
  std::shared_future<int> port = portP.get_future().share();
  std::vector<std::string> err(static_cast<size_t>(N), std::string());
  auto run = [&](int r) {
    try {
      TcpCtrl c(r, N);
      if (r == 0) portP.set_value(c.listen(0, "127.0.0.1"));
      c.connect("127.0.0.1", port.get(), 30.0);
      body(r, c);
    } catch (const std::exception &e) {
      err[size_t(r)] = e.what();
      if (r == 0) {
        try {
          portP.set_value(-1);
        } catch (...) {
        }
      }
    }
  };
  std::vector<std::thread> ts;
  for (int r = 0; r < N; ++r) ts.emplace_back(run, r);
  for (auto &t : ts) t.join();
  return err;
}

TEST(tcp_ctrl_alltoallv_and_transport_health) {
  // round-3 control-plane additions with ranks as threads (the TSan build checks them for data
  // races): the personalized exchange of the host-staged transport, the collective agreement on
  // dead ordering domains, and the recovery hooks that run on every rank after an aborted run
  constexpr int N = 3;
  revive_domains();
  std::atomic<int> hookRuns{0};
  const int hook = add_recovery_hook([&](Ctrl &c) {
    ++hookRuns;
    c.barrier(); // hooks are collective
  });
  std::vector<std::vector<std::string>> got(N);
  std::vector<std::set<std::string>> dead(N);
  std::vector<int> rec1(N, -1), rec2(N, -1);
  auto err = tcp_ranks(N, [&](int r, TcpCtrl &c) {
    std::vector<std::string> out(N);
    for (int q = 0; q < N; ++q)
      out[size_t(q)] = (q == r) ? "" : std::string(size_t(1000 * (r + 1)), char('a' + r)) + "->" + std::to_string(q);
    got[size_t(r)] = c.alltoallv(out);
    if (r == 1) mark_domain_dead("rccl", "unit test");
    if (r == 2) note_abort();
    c.barrier();
    dead[size_t(r)] = agree_dead_domains(c);
    rec1[size_t(r)] = recover_after_abort(c) ? 1 : 0;
    c.barrier();
    rec2[size_t(r)] = recover_after_abort(c) ? 1 : 0;
  });
  remove_recovery_hook(hook);
  for (int r = 0; r < N; ++r) {
    if (!err[size_t(r)].empty()) std::fprintf(stderr, "  rank %d: %s\n", r, err[size_t(r)].c_str());
    CHECK(err[size_t(r)].empty());
    CHECK(got[size_t(r)].size() == size_t(N));
    for (int q = 0; q < N && got[size_t(r)].size() == size_t(N); ++q) {
      const std::string want =
          q == r ? "" : std::string(size_t(1000 * (q + 1)), char('a' + q)) + "->" + std::to_string(r);
      CHECK(got[size_t(r)][size_t(q)] == want);
    }
    CHECK(dead[size_t(r)].count("rccl") == 1);
    CHECK(rec1[size_t(r)] == 1); // rank 2 aborted a run: every rank recovers
    CHECK(rec2[size_t(r)] == 0); // nothing new since
  }
  CHECK(hookRuns.load() == N);
  CHECK(domain_dead("rccl"));
  revive_domains();
  CHECK(!domain_dead("rccl") && dead_domains().empty());
}

namespace {
/// forwards to a control plane and records the collectives made through it: 'b' barrier,
/// 'm' allreduce_max, '?' anything else
class CountingCtrl : public Ctrl {
public:
  explicit CountingCtrl(Ctrl &c) : c_(c) {}
  std::string calls;
  int rank() const override { return c_.rank(); }
  int size() const override { return c_.size(); }
  void barrier() override {
    calls += 'b';
    c_.barrier();
  }
  void bcast(std::string &d, int root) override {
    calls += '?';
    c_.bcast(d, root);
  }
  void allreduce_max(double *v, size_t n) override {
    calls += n == 1 ? 'm' : '?';
    c_.allreduce_max(v, n);
  }
  void allreduce_sum(double *v, size_t n) override {
    calls += '?';
    c_.allreduce_sum(v, n);
  }
  std::vector<std::string> allgather(const std::string &mine) override {
    calls += '?';
    return c_.allgather(mine);
  }

private:
  Ctrl &c_;
};
} // namespace

TEST(agree_keeps_the_local_reason) {
  constexpr int N = 3;
  std::vector<std::vector<std::string>> got(N);
  auto err = tcp_ranks(N, [&](int r, TcpCtrl &c) {
    got[size_t(r)].push_back(agree(c, ""));                                  // everyone passes
    got[size_t(r)].push_back(agree(c, r == 1 ? "disk full" : ""));           // one local reason
    got[size_t(r)].push_back(agree(c, r == 2 ? "no link" : "", "elsewhere")); // the foreign text
    got[size_t(r)].push_back(agree(c, "rank " + std::to_string(r)));         // everyone fails
  });
  for (int r = 0; r < N; ++r) {
    CHECK(err[size_t(r)].empty());
    CHECK(got[size_t(r)].size() == 4);
    if (got[size_t(r)].size() != 4) continue;
    CHECK(got[size_t(r)][0].empty());
    CHECK(got[size_t(r)][1] == (r == 1 ? "disk full" : "failed on another rank"));
    CHECK(got[size_t(r)][2] == (r == 2 ? "no link" : "elsewhere"));
    CHECK(got[size_t(r)][3] == "rank " + std::to_string(r));
  }
}

TEST(agreed_trial_keeps_ranks_in_step_whatever_fails) {
  // a sequence of trials in which nobody fails, then an exchange throws on rank 1, a verify
  // returns a reason on rank 2, a verify throws on rank 0, and rank 1 is failed by
  // TZ_FAIL_TRANSPORTS (its trial is named after the rank: the ranks are threads of one process
  // and share the environment). The sequence completing at all shows that no outcome leaves the
  // ranks in mismatched collectives; the counting control plane shows the one barrier followed
  // by one allreduce_max per trial.
  constexpr int N = 3, T = 5;
  ::setenv("TZ_FAIL_TRANSPORTS", "other,sim_r1", 1);
  CHECK(fail_simulated("sim_r1") && fail_simulated("other") && !fail_simulated("sim_r") &&
        !fail_simulated("sim_r2") && !fail_simulated(""));
  std::vector<std::vector<std::string>> got(N);
  std::vector<std::string> calls(N);
  std::vector<std::vector<int>> verified(N, std::vector<int>(T, 0));
  auto err = tcp_ranks(N, [&](int r, TcpCtrl &tcp) {
    CountingCtrl c(tcp);
    for (int t = 0; t < T; ++t) {
      const std::string name = t == 4 ? "sim_r" + std::to_string(r) : "trial" + std::to_string(t);
      got[size_t(r)].push_back(agreed_trial(
          c, name,
          [&] {
            if (t == 1 && r == 1) throw std::runtime_error("exchange broke");
          },
          [&]() -> std::string {
            ++verified[size_t(r)][size_t(t)];
            if (t == 2 && r == 2) return name + " preflight: 7 wrong cells";
            if (t == 3 && r == 0) throw std::runtime_error("check broke");
            return "";
          }));
    }
    calls[size_t(r)] = c.calls;
  });
  ::unsetenv("TZ_FAIL_TRANSPORTS");
  const int failing[T] = {-1, 1, 2, 0, 1};
  const std::string own[T] = {"", "trial1: exchange broke", "trial2 preflight: 7 wrong cells",
                              "trial3 check: check broke", "sim_r1: simulated failure (TZ_FAIL_TRANSPORTS)"};
  for (int r = 0; r < N; ++r) {
    if (!err[size_t(r)].empty()) std::fprintf(stderr, "  rank %d: %s\n", r, err[size_t(r)].c_str());
    CHECK(err[size_t(r)].empty());
    CHECK(calls[size_t(r)] == "bmbmbmbmbm");
    CHECK(got[size_t(r)].size() == size_t(T));
    for (int t = 0; t < T && got[size_t(r)].size() == size_t(T); ++t) {
      const std::string &g = got[size_t(r)][size_t(t)];
      if (failing[t] < 0) CHECK(g.empty());
      else CHECK(g == (failing[t] == r ? own[t] : "failed on another rank"));
      // verify runs exactly where the rank's own exchange did not throw
      CHECK(verified[size_t(r)][size_t(t)] == (t == 1 && r == 1 ? 0 : 1));
    }
  }
}

TEST(ipc_blob_layout) {
  // the exported blob with 64-byte opaque handles: [node identity][handles][payload]
  constexpr size_t H = 64;
  const std::string node = std::string("host-a|boot-1") + std::string(83, '\0');
  const std::string other = std::string("host-b|boot-1") + std::string(83, '\0');
  auto hnd = [&](char c) { return std::string(H, c); };
  auto throws = [](const std::function<void()> &f, const char *what) {
    try {
      f();
    } catch (const std::exception &e) {
      return std::string(e.what()).find(what) != std::string::npos;
    }
    return false;
  };
  const std::string blob = ipc_blob::pack(node, {hnd('a'), hnd('b'), hnd('c')}, "payload!");
  CHECK(blob.size() == node.size() + 3 * H + 8);
  CHECK(ipc_blob::handle(blob, node, H, 0) == hnd('a'));
  CHECK(ipc_blob::handle(blob, node, H, 1) == hnd('b'));
  CHECK(ipc_blob::handle(blob, node, H, 2) == hnd('c'));
  CHECK(ipc_blob::payload(blob, node.size(), H, 3) == "payload!");
  // a blob too short for the slot (a peer that failed to export sends an empty one)
  const std::string two = ipc_blob::pack(node, {hnd('a'), hnd('b')});
  CHECK(ipc_blob::handle(two, node, H, 1) == hnd('b'));
  CHECK(throws([&] { ipc_blob::handle(two, node, H, 2); }, "exported no IPC handles"));
  CHECK(throws([&] { ipc_blob::handle(two.substr(0, two.size() - 1), node, H, 1); }, "exported no IPC handles"));
  CHECK(throws([&] { ipc_blob::handle("", node, H, 0); }, "exported no IPC handles"));
  CHECK(throws([&] { ipc_blob::payload(two, node.size(), H, 3); }, "exported no IPC handles"));
  // a handle from another node is never opened
  CHECK(throws([&] { ipc_blob::handle(blob, other, H, 0); }, "another node"));
  // an all-zero slot is rejected, its neighbours open
  const std::string gap = ipc_blob::pack(node, {hnd('a'), std::string(H, '\0'), hnd('c')});
  CHECK(ipc_blob::handle(gap, node, H, 0) == hnd('a'));
  CHECK(throws([&] { ipc_blob::handle(gap, node, H, 1); }, "no IPC handle in slot 1"));
  CHECK(ipc_blob::handle(gap, node, H, 2) == hnd('c'));
  // a single non-zero byte makes a handle
  std::string one(H, '\0');
  one[H - 1] = 1;
  CHECK(ipc_blob::handle(ipc_blob::pack(node, {one}), node, H, 0) == one);
  // no handles at all: the payload starts right behind the node identity
  CHECK(ipc_blob::payload(ipc_blob::pack(node, {}, "xyz"), node.size(), H, 0) == "xyz");
  CHECK(ipc_blob::payload(ipc_blob::pack(node, {}), node.size(), H, 0).empty());
}

TEST(ordering_domain_orders_ops_across_streams) {
  // two independent ops of one ordering domain (like two RCCL groups on different
  // communicators) never run unordered: whatever streams the schedule puts them on, the later
  // one waits for the earlier (an implicit edge the synchronizer covers and verify() checks)
  auto g = std::make_shared<Graph>();
  auto a = std::make_shared<SimGpuOp>("a", 10, "rccl");
  auto b = std::make_shared<SimGpuOp>("b", 10, "rccl");
  auto c = std::make_shared<SimGpuOp>("c", 10); // no domain: free to overlap
  for (auto &op : std::vector<OpPtr>{a, b, c}) {
    g->start_then(op);
    g->then_finish(op);
  }
  std::mt19937_64 rng(7);
  int ordered = 0;
  for (int seed = 0; seed < 40; ++seed) {
    State s(g, Platform::make_n_streams(3));
    Sequence seq = random_rollout(s, rng);
    CHECK(verify(seq, *g, 3).empty());
    // count the schedules whose two domain ops landed on different streams
    int sa = -1, sb = -1;
    for (size_t k = 0; k < seq.size(); ++k) {
      const auto *op = dynamic_cast<const BoundGpuOp *>(seq[k].get());
      if (op && op->name() == "a") sa = op->stream();
      if (op && op->name() == "b") sb = op->stream();
    }
    ordered += sa != sb;
  }
  CHECK(ordered > 0); // some schedules split them over streams, and those verified too
  // negative control: a and b on two streams with nothing between them is a violation (no
  // graph edge joins them; the domain does), c on a third stream is not
  Graph ng = *g;
  ng.normalize();
  auto k = [&](const char *n) { return std::static_pointer_cast<const GpuOp>(ng.op(ng.find(n))); };
  Sequence s;
  s.push_back(std::make_shared<Start>());
  s.push_back(std::make_shared<BoundGpuOp>(k("a"), 0));
  s.push_back(std::make_shared<BoundGpuOp>(k("b"), 1));
  s.push_back(std::make_shared<BoundGpuOp>(k("c"), 2));
  s.push_back(std::make_shared<StreamSync>(0));
  s.push_back(std::make_shared<StreamSync>(1));
  s.push_back(std::make_shared<StreamSync>(2));
  s.push_back(std::make_shared<Finish>());
  CHECK(verify(s, ng, 3).size() == 1);
  Sequence f = s;
  f.entries.insert(f.entries.begin() + 2, SeqEntry{std::make_shared<EventRecord>(0, 0)});
  f.entries.insert(f.entries.begin() + 3, SeqEntry{std::make_shared<StreamWaitEvent>(1, 0)});
  CHECK(verify(f, ng, 3).empty());
}

TEST(run_deadline_arms_and_cancels) {
  // the run deadline (bench.py, tz-search --deadline) prints its report and exits when it
  // fires; here only arming, the remaining time and cancelling are checked (firing would end
  // this process: the Python suite covers it in a child process)
  RunDeadline d(30.0, 5);
  CHECK(d.armed());
  const double left = d.remaining();
  CHECK(left > 25.0 && left <= 30.0);
  d.set_report("{\"partial\": true}");
  std::this_thread::sleep_for(std::chrono::milliseconds(20));
  CHECK(d.remaining() < left);
  d.cancel();
  CHECK(!d.armed());
}

TEST(deadline_claim_run_ends_at_its_deadline) {
  // a run that finishes right at its deadline must be either aborted or not, never
  // half: the watchdog's claim succeeds iff the run's finish reports the abort
  DeadlineClaim c;
  CHECK(!c.try_claim(1.0)); // nothing armed
  c.arm(10.0);
  CHECK(!c.try_claim(9.0)); // not expired
  CHECK(!c.finish());        // ended in time
  CHECK(c.value() == 0);
  CHECK(!c.try_claim(11.0)); // ended: nothing to claim
  c.arm(10.0);
  CHECK(c.try_claim(10.5));
  CHECK(!c.try_claim(10.6)); // claimed once
  CHECK(c.abort_pending());
  CHECK(c.finish());
  CHECK(c.abort_pending()); // draining
  c.drained();
  CHECK(!c.abort_pending() && c.value() == 0);
  // the race: the waiter ends exactly while the watchdog sweeps past the deadline, many times
  int claimed = 0, reported = 0, mismatched = 0;
  for (int it = 0; it < 20000; ++it) {
    DeadlineClaim r;
    r.arm(1.0); // already expired for the watchdog (now = 2.0)
    std::atomic<bool> go{false};
    bool won = false;
    std::thread wd([&] {
      while (!go.load()) {
      }
      won = r.try_claim(2.0);
    });
    go = true;
    const bool aborted = r.finish();
    wd.join();
    claimed += won;
    reported += aborted;
    mismatched += won != aborted;
    if (aborted) r.drained();
    CHECK(r.value() == 0);
  }
  CHECK(mismatched == 0);
  CHECK(claimed == reported);
  std::printf("  deadline race: %d of 20000 ends claimed by the watchdog, all reported\n", claimed);
}

TEST(deadline_claim_abort_pending_through_finish) {
  // between a claimed wait's end and its drain, a watchdog sweep must always see the
  // abort pending (never the 0 of a finished wait), or a drain that hangs loses its grace exit
  std::atomic<int> seen0{0}, sweeps{0};
  for (int it = 0; it < 2000; ++it) {
    DeadlineClaim c;
    c.arm(1.0);
    CHECK(c.try_claim(2.0));
    std::atomic<bool> stop{false}, running{false};
    std::thread wd([&] {
      while (!stop.load()) {
        ++sweeps;
        if (!c.abort_pending()) ++seen0;
        running = true;
      }
    });
    while (!running.load()) {
    }
    const bool aborted = c.finish();
    CHECK(aborted);
    CHECK(c.abort_pending() && c.value() == DeadlineClaim::kDraining);
    stop = true;
    wd.join();
    c.drained();
    CHECK(!c.abort_pending());
  }
  CHECK(seen0 == 0);
  CHECK(sweeps > 0);
  std::printf("  %d watchdog sweeps during claimed finishes, none saw the wait as ended\n", sweeps.load());
}

TEST(runs_test_behaviour) {
  std::vector<double> alt, trend;
  for (int i = 0; i < 40; ++i) {
    alt.push_back(i % 2 ? 1.0 : 2.0);
    trend.push_back(double(i));
  }
  CHECK(runs_test(trend));   // monotone trend: non-random
  CHECK(runs_test(alt));     // perfectly alternating: non-random
  std::vector<double> small{1, 2, 3};
  CHECK(!runs_test(small, RunsTestSmall::Accept));
  CHECK(runs_test(small, RunsTestSmall::Reject)); // reference behaviour
  auto pf = prime_factors(24);
  CHECK(pf.size() == 4 && pf[0] == 3 && pf[3] == 2);
}

int main(int argc, char **argv) {
  const char *filter = argc > 1 ? argv[1] : nullptr;
  int ran = 0;
  for (auto &c : cases()) {
    if (filter && !std::strstr(c.name, filter)) continue;
    const int before = g_fail;
    try {
      c.fn();
    } catch (const std::exception &e) {
      ++g_fail;
      std::fprintf(stderr, "  EXCEPTION in %s: %s\n", c.name, e.what());
    }
    std::fprintf(stderr, "[%s] %s\n", g_fail == before ? " ok " : "FAIL", c.name);
    ++ran;
  }
  std::fprintf(stderr, "%d test cases, %d checks, %d failures\n", ran, g_checks, g_fail);
  return g_fail ? 1 : 0;
}
