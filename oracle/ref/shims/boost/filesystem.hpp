/* Stand-in for <boost/filesystem.hpp>: exists, path, parent_path, is_absolute, operator/ and wstring are all the reference
 * uses of it in the files the recipe builds, and std::filesystem has them under the same names. */
#pragma once
#include <filesystem>

namespace boost {
namespace filesystem = std::filesystem;
}
