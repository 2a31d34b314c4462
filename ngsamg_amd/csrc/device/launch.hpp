// Typed kernel dispatch: a run-time value picks one template instantiation out of a list written at the call site.
//
//   auto run = [&](auto G) { launch(sell_spmv_kernel<G(), EP>, grid, BLOCK, 0, stream, args...); };
//   if (!dispatch<1, 2, 4, 8>(M.lanes, run)) run(Int<16>{});        // any other lane count: the 16-lane kernel
//
// Exactly the listed values (and a fallback that is written out) are instantiated; combinations a kernel is not built for are
// kept out with `if constexpr` inside the lambda.
#pragma once
#include <array>
#include <type_traits>

namespace amgx {

template <int V> using Int = std::integral_constant<int, V>;

// calls f(Int<Vi>{}) for the one Vi == value; false (and no call) when value is not in the list
template <int... Vs, class F>
bool dispatch(int value, F&& f) {
  return ((value == Vs ? (f(Int<Vs>{}), true) : false) || ...);
}

// a value list with a name: the same list then serves the dispatch and the question whether a kernel exists
//   using SquareShapes = IntList<22, 33, 66>;     dispatch(SquareShapes{}, key, run)     contains(SquareShapes{}, key)
template <int... Vs> struct IntList {};
template <int... Vs, class F>
bool dispatch(IntList<Vs...>, int value, F&& f) { return dispatch<Vs...>(value, static_cast<F&&>(f)); }
template <int... Vs>
constexpr bool contains(IntList<Vs...>, int value) { return ((value == Vs) || ...); }
// ... and a builder that tries the values in their order:     for (int g : values(DownLwLanes{}))
template <int... Vs>
constexpr std::array<int, sizeof...(Vs)> values(IntList<Vs...>) { return {{Vs...}}; }

}  // namespace amgx

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#include <stdexcept>
#include <string>

namespace amgx {

struct Err : std::runtime_error { using std::runtime_error::runtime_error; };

#define HIPCHK(call)                                                                                  \
  do {                                                                                                \
    hipError_t e_ = (call);                                                                           \
    if (e_ != hipSuccess)                                                                             \
      throw ::amgx::Err(std::string(#call) + " failed: " + hipGetErrorString(e_) + " (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
  } while (0)

// kernel<<<grid, block, lds_bytes, stream>>>(args...), then the launch error as an Err.  The arguments convert to the kernel's
// parameter types as they do at a direct call (std::common_type_t keeps them out of the deduction).
template <class... P>
void launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, std::common_type_t<P>... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, args...);
  HIPCHK(hipGetLastError());
}

}  // namespace amgx
#endif
