// walk_nodes_check.cpp — TEST INFRASTRUCTURE: a stand-alone program over walk_facts of csrc/scene_facts.h with its node
// output, for tests/test_walk_nodes.py to build with -fsanitize=address,undefined and run.  Reads trees from the file named
// by its argument, each as {u32 nodes, u32 root, u32 cap, nodes x 8 words}; gives walk_facts heap arrays of exactly the
// sizes it asks for (kMaxLeafRecords, kMaxNodeRecords), so that a record written past either is an error of the sanitizer;
// checks what a sweep relies on and prints one line per tree: "<sweepable> <leaves> <nodes>".
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../webgpu-raytracer_amd/csrc/scene_facts.h"

static int fail(const char* what, size_t tree) {
  std::fprintf(stderr, "tree %zu: %s\n", tree, what);
  return 1;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[3];
  for (size_t tree = 0; std::fread(head, 4, 3, f) == 3; tree++) {
    std::vector<rt_node> blas(head[0]);
    static_assert(sizeof(rt_node) == 32, "a node is 8 words");
    if (std::fread(blas.data(), 32, blas.size(), f) != blas.size()) return 2;
    std::unique_ptr<scene_facts::LeafRecord[]> leaves(new scene_facts::LeafRecord[scene_facts::kMaxLeafRecords]);
    std::unique_ptr<scene_facts::NodeRecord[]> nodes(new scene_facts::NodeRecord[scene_facts::kMaxNodeRecords]);
    uint32_t n_nodes = 0xffffffffu;
    const launch_plan::WalkFacts w =
        scene_facts::walk_facts(blas.data(), blas.size(), head[1], head[2], leaves.get(), nodes.get(), &n_nodes);
    // the old signature gives the same verdict and the same leaves
    std::unique_ptr<scene_facts::LeafRecord[]> leaves2(new scene_facts::LeafRecord[scene_facts::kMaxLeafRecords]);
    const launch_plan::WalkFacts w2 = scene_facts::walk_facts(blas.data(), blas.size(), head[1], head[2], leaves2.get());
    if (w.known != w2.known || w.sweepable != w2.sweepable || w.n_leaves != w2.n_leaves) return fail("the two signatures disagree", tree);
    if (!w.sweepable) {
      if (n_nodes != 0u) return fail("nodes of a tree that is not sweepable", tree);
      std::printf("0 0 0\n");
      continue;
    }
    if (std::memcmp(leaves.get(), leaves2.get(), w.n_leaves * sizeof(scene_facts::LeafRecord)) != 0)
      return fail("the two signatures' leaves differ", tree);
    if (n_nodes < w.n_leaves || n_nodes > 2u * w.n_leaves - 1u || n_nodes > scene_facts::kMaxNodeRecords)
      return fail("node count", tree);
    uint32_t l = 0;
    for (uint32_t i = 0; i < n_nodes; i++) {
      const scene_facts::NodeRecord& r = nodes[i];
      if (r.data == 0u) {
        if (r.div < i + 3u || r.div > n_nodes) return fail("an inner record's subtree end", tree);
      } else {
        if (l >= w.n_leaves || std::memcmp(&r, &leaves[l], sizeof r) != 0) return fail("a leaf record differs from the leaf array's", tree);
        l++;
      }
    }
    if (l != w.n_leaves) return fail("leaves among the nodes", tree);
    std::printf("1 %u %u\n", w.n_leaves, n_nodes);
  }
  std::fclose(f);
  // no outputs asked for, or no room to say how many nodes: nothing is written, nothing is sweepable
  rt_node one = {};
  one.max_b[0] = one.max_b[1] = one.max_b[2] = 1.0f;
  one.skip = 1u;
  one.data = 1u;
  scene_facts::LeafRecord leaf;
  scene_facts::NodeRecord node;
  if (scene_facts::walk_facts(&one, 1, 0, 16, nullptr).known) return fail("no leaf output", 0);
  if (scene_facts::walk_facts(&one, 1, 0, 16, &leaf, &node, nullptr).sweepable) return fail("nodes without their count", 0);
  uint32_t n = 7;
  if (!scene_facts::walk_facts(&one, 1, 0, 16, &leaf, &node, &n).sweepable || n != 1u) return fail("a root that is a leaf", 0);
  std::printf("ok\n");
  return 0;
}
