/* Forced in front of every reference file the recipe compiles (-include): the standard headers those files use without
 * including them (they lean on what the MSVC headers pull in), and an assert that takes the message the reference passes as
 * a second argument.  A failed assert reports and aborts: the probe never runs past one. */
#pragma once
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
/* The reference calls abs() unqualified on floats (AABB.cpp, Vector.cpp).  MSVC's headers give the global abs its float
 * overloads; with <cstdlib> alone g++ finds only abs(int) and TRUNCATES the argument (a triangle's bounding box would shrink to
 * whole units).  libstdc++'s <math.h> and <stdlib.h> bring std::abs's overloads into the global namespace. */
#include <math.h>
#include <stdlib.h>

#undef assert
#define assert(cond, ...) ((cond) ? (void)0 : (std::fprintf(stderr, "reference assert failed: %s (%s:%d)\n", #cond, __FILE__, __LINE__), std::abort()))
