// kino_heap.h — the open set of KinoAstar::search (kino_astar.h:136) as libstdc++ runs it, for host and device.
//
// The reference's open set is std::priority_queue<PathNode*, std::vector<PathNode*>, NodeComparator> with the comparator
// `node1->f_score > node2->f_score` (kino_astar.h:67-73).  It holds POINTERS, and the search lowers the f_score of a node that
// is still in the queue in place, without re-heapifying (kino_astar.cpp:276-289): later pushes and pops run libstdc++'s heap
// algorithms on an array that may no longer be a heap, comparing the nodes' CURRENT keys.  Which node comes out on top — ties
// in f included — is therefore a property of those exact algorithms, not of "a priority queue".  This restates them
// (bits/stl_heap.h):
//   push:  push_back, then __push_heap(first, len - 1, 0, value): sift the hole up while comp(parent, value);
//   pop:   __pop_heap(first, last - 1, last - 1): the last element is taken out as `value`, the top moves to the end,
//          __adjust_heap(first, 0, len - 1, value): the hole walks down to a leaf through the child that is not "less"
//          (the right child unless comp(right, left)), the lone left child at the bottom when len is even, then
//          __push_heap from there back up towards 0; then pop_back.  A queue of one element is only popped.
// A pointer dereference becomes a cached key beside each entry: key[i] is the current f of node[i], and set_key rewrites it
// where the node stands (pos[node]), which is exactly what the reference's comparator would read afterwards.
#pragma once
#include "device_types.h"

namespace dftpav {

struct KinoHeap {
  int *node;   // [cap] node index of each entry
  double *key; // [cap] its current f
  int *pos;    // [number of nodes] entry of each node (valid while the node is in the heap)
  int size;

  // comp(a, b) of NodeComparator: a->f_score > b->f_score
  DFTPAV_HD static bool comp(double a, double b) { return a > b; }

  DFTPAV_HD void place(int i, int n, double k) {
    node[i] = n;
    key[i] = k;
    pos[n] = i;
  }
  // std::__push_heap(first, hole, top, value, comp)
  DFTPAV_HD void push_up(int hole, int top, int vn, double vk) {
    int parent = (hole - 1) / 2;
    while (hole > top && comp(key[parent], vk)) {
      place(hole, node[parent], key[parent]);
      hole = parent;
      parent = (hole - 1) / 2;
    }
    place(hole, vn, vk);
  }
  // std::__adjust_heap(first, hole, len, value, comp)
  DFTPAV_HD void adjust(int hole, int len, int vn, double vk) {
    const int top = hole;
    int second = hole;
    while (second < (len - 1) / 2) {
      second = 2 * (second + 1);
      if (comp(key[second], key[second - 1])) second--;
      place(hole, node[second], key[second]);
      hole = second;
    }
    if ((len & 1) == 0 && second == (len - 2) / 2) {
      second = 2 * (second + 1);
      place(hole, node[second - 1], key[second - 1]);
      hole = second - 1;
    }
    push_up(hole, top, vn, vk);
  }
  DFTPAV_HD int top() const { return node[0]; }
  DFTPAV_HD bool empty() const { return size == 0; }
  DFTPAV_HD void push(int n, double k) {
    size++;
    push_up(size - 1, 0, n, k);
  }
  DFTPAV_HD void pop() {
    if (size > 1) { // std::pop_heap: __pop_heap(first, last - 1, last - 1)
      const int last = size - 1;
      const int vn = node[last];
      const double vk = key[last];
      place(last, node[0], key[0]);
      adjust(0, last, vn, vk);
    }
    size--;
  }
  // pro_node->f_score = tmp_f_score on a node in the open set (kino_astar.cpp:284): no re-heapify
  DFTPAV_HD void set_key(int n, double k) { key[pos[n]] = k; }
};

} // namespace dftpav
