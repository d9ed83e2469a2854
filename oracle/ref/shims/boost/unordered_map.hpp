/* Stand-in for <boost/unordered_map.hpp>: the reference only declares maps, indexes them, calls find / at / size and iterates.
 * Iteration order is std::unordered_map's; the .vox readers are order-agnostic (tests/test_voxelizer.py). */
#pragma once
#include <unordered_map>

namespace boost {
template <class K, class V, class H = std::hash<K>, class E = std::equal_to<K>>
using unordered_map = std::unordered_map<K, V, H, E>;
}
