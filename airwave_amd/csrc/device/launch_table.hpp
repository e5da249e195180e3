// launch_table.hpp — host side of a kernel family: one table row per template instantiation the library carries.  A family's table
// is the only place that says which instantiations exist; preparing (dynamic-LDS attribute), "is there a kernel for this layout",
// the kernel's name and its launch all read that table.  Tables are built from the X-macro lists next to the kernels, one row macro each.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace awk {

template <class... A>
struct KernelEntry {
    int key;                 // what the launcher looks a kernel up by: channels, pairs, (channels, rows) ... packed by the table's owner
    void (*fn)(A...);        // the __global__ instantiation
    int lds_bytes;           // dynamic LDS of a launch
    const char *name;
};

// Kernels that use more than 64 KB of dynamic LDS need the attribute before their first launch: every row of a table, once per context.
template <class... A, size_t N>
hipError_t set_dynamic_lds(const KernelEntry<A...> (&table)[N]) {
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < N && e == hipSuccess; ++i)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(table[i].fn), hipFuncAttributeMaxDynamicSharedMemorySize, table[i].lds_bytes);
    return e;
}

// nullptr: the library carries no such kernel
template <class... A, size_t N>
const KernelEntry<A...> *find(const KernelEntry<A...> (&table)[N], int key) {
    for (const KernelEntry<A...> &k : table)
        if (k.key == key) return &k;
    return nullptr;
}

template <class... A>
void launch(const KernelEntry<A...> &k, dim3 grid, dim3 block, hipStream_t stream, A... args) {
    hipLaunchKernelGGL(k.fn, grid, block, k.lds_bytes, stream, args...);
}

}  // namespace awk
