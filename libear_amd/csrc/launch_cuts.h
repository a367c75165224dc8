// launch_cuts.h — the two bits of arithmetic every output-bus stage repeats, as plain C++ (the CPU tests compile it): a call cut
// into launches, and which half of a two-halves buffer is read and which is written.
#pragma once

#include <algorithm>
#include <cstddef>

namespace earhip {

// f(at, n) for the pieces of [0, total) in order: each of `most`, the last of what is left.  f returns how far the output moved.
template <typename F>
void for_each_launch(size_t total, size_t most, F &&f) {
  size_t out_at = 0;
  for (size_t at = 0; at < total;) {
    const size_t n = std::min(most, total - at);
    out_at += f(at, n, out_at);
    at += n;
  }
}

// a buffer of two halves: a launch reads the state in one and writes the next state to the other
struct Halves {
  size_t half = 0;
  int par = 0;  // the half that holds the state in front of the next launch
  size_t in() const { return (size_t)par * half; }
  size_t out() const { return (size_t)(par ^ 1) * half; }
  void flip() { par ^= 1; }
};

}  // namespace earhip
