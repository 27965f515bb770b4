// cluster_unionfind_host.cpp -- csrc/cloud_unionfind.h as host C++: the two functions mvs_cloud_cluster's union launch
// runs, from 16 threads on one parent array, built with the address and undefined-behaviour sanitizers by
// tests/test_cloud_cluster_host.py.  No GPU, nothing loaded into Python.
//
// The graphs: a line of N points (edges i -- i + 1: one set, 2,000 hops across), the same line under a shuffle and under an
// even / odd interleave of the indices, a random graph of many small and one large component, no edges at all, and two
// lines of 300,000 points, long enough for the threads to meet on the same words.  The threads wait for each other before
// the first union.  The edges are dealt to the threads round robin
// and in a per-thread shuffled order, every edge is also united a second time by another thread, and finds run between
// the unions.  Checked after the join: every parent word is <= its index (the invariant), the root of every point is the
// smallest index of its component (computed by a sequential flood fill), and a root's word names itself.  A find that
// did not end would end the test at its time limit, on the CPU.
#include "cloud_unionfind.h"

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <utility>
#include <vector>

namespace {

constexpr int kThreads = 16;
using Edge = std::pair<unsigned, unsigned>;

struct Rng {      // SplitMix64: the same stream everywhere
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    unsigned below(unsigned n) { return (unsigned)(next() % n); }
};

template <typename T>
void shuffle(std::vector<T>& v, Rng& rng) {
    for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[rng.below((unsigned)i)]);
}

// the smallest index of every point's component, by a flood fill from the points in ascending order
std::vector<unsigned> component_min(unsigned n, const std::vector<Edge>& edges) {
    std::vector<std::vector<unsigned>> adj(n);
    for (const Edge& e : edges) {
        adj[e.first].push_back(e.second);
        adj[e.second].push_back(e.first);
    }
    std::vector<unsigned> low(n, UINT32_MAX), stack;
    for (unsigned s = 0; s < n; ++s) {
        if (low[s] != UINT32_MAX) continue;
        low[s] = s;
        stack.push_back(s);
        while (!stack.empty()) {
            const unsigned x = stack.back();
            stack.pop_back();
            for (unsigned y : adj[x])
                if (low[y] == UINT32_MAX) {
                    low[y] = s;
                    stack.push_back(y);
                }
        }
    }
    return low;
}

long long run(const char* what, unsigned n, const std::vector<Edge>& edges, uint64_t seed) {
    std::vector<unsigned> parent(n);
    for (unsigned i = 0; i < n; ++i) parent[i] = i;
    std::vector<std::thread> pool;
    std::atomic<int> ready{0};      // the threads start uniting together, each with its edges already dealt
    for (int t = 0; t < kThreads; ++t)
        pool.emplace_back([&, t] {
            Rng rng{seed * 1000 + (uint64_t)t};
            std::vector<Edge> mine;
            for (size_t k = 0; k < edges.size(); ++k)
                if ((int)(k % kThreads) == t || (int)((k + 5) % kThreads) == t) mine.push_back(edges[k]);
            shuffle(mine, rng);
            ready.fetch_add(1);
            while (ready.load() < kThreads) std::this_thread::yield();
            for (const Edge& e : mine) {
                if (rng.below(2)) mvs::uf_union(parent.data(), e.first, e.second);
                else mvs::uf_union(parent.data(), e.second, e.first);
                const unsigned x = rng.below(n);
                if (mvs::uf_find(parent.data(), x) > x) std::abort();      // a root above its point
            }
        });
    for (std::thread& th : pool) th.join();
    const std::vector<unsigned> low = component_min(n, edges);
    long long bad = 0, sets = 0;
    for (unsigned i = 0; i < n; ++i) {
        if (parent[i] > i) ++bad;
        if (mvs::uf_root(parent.data(), i) != low[i]) ++bad;
        if (mvs::uf_find(parent.data(), i) != low[i]) ++bad;
        if (low[i] == i) {
            ++sets;
            if (parent[i] != i) ++bad;
        }
    }
    std::printf("%s: %u points, %zu edges, %lld sets, %lld bad\n", what, n, edges.size(), sets, bad);
    return bad;
}

}  // namespace

int main() {
    long long bad = 0;
    const unsigned N = 2000;
    std::vector<Edge> line;
    for (unsigned i = 0; i + 1 < N; ++i) line.push_back({i, i + 1});
    bad += run("line", N, line, 1);
    std::reverse(line.begin(), line.end());
    bad += run("line, edges descending", N, line, 2);
    Rng rng{3};
    std::vector<unsigned> perm(N);
    for (unsigned i = 0; i < N; ++i) perm[i] = i;
    shuffle(perm, rng);
    std::vector<Edge> shuffled;
    for (unsigned i = 0; i + 1 < N; ++i) shuffled.push_back({perm[i], perm[i + 1]});
    bad += run("shuffled line", N, shuffled, 4);
    // even / odd interleave: the points 0, 2, 4, ... then 1, 3, 5, ... along the line
    std::vector<Edge> interleaved;
    for (unsigned i = 0; i + 1 < N; ++i) {
        auto at = [&](unsigned k) { return k % 2 ? N / 2 + k / 2 : k / 2; };
        interleaved.push_back({at(i), at(i + 1)});
    }
    bad += run("interleaved line", N, interleaved, 5);
    // a random graph: 20,000 points, 12,000 edges among them (many small sets, singletons), plus one set of 3,000 points
    const unsigned M = 20000;
    std::vector<Edge> graph;
    for (int k = 0; k < 12000; ++k) graph.push_back({rng.below(M), rng.below(M)});
    for (int k = 0; k < 6000; ++k) graph.push_back({17000 + rng.below(3000), 17000 + rng.below(3000)});
    bad += run("random graph", M, graph, 6);
    bad += run("no edges", 100, {}, 7);
    // long enough for the 16 threads to meet on the same words
    std::vector<Edge> longline;
    for (unsigned i = 0; i + 1 < 300000; ++i) longline.push_back({i, i + 1});
    bad += run("long line", 300000, longline, 8);
    shuffle(longline, rng);
    for (Edge& e : longline) e = {(unsigned)((e.first * 7919ull) % 300000), (unsigned)((e.second * 7919ull) % 300000)};
    bad += run("long line, indices permuted", 300000, longline, 9);
    std::printf("total: %lld bad\n", bad);
    return bad ? 1 : 0;
}
