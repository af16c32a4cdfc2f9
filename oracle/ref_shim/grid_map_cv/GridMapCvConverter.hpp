// Functional stand-in (TEST INFRASTRUCTURE): our own text, just enough of the third-party names for the reference's
// GroundSegmentation translation unit to compile unmodified and run (oracle/ref_build.py).  It is not the library it is named after,
// builds no other part of the reference and pins no third-party arithmetic (tools/pin/ does that).
// grid_map_cv/GridMapCvConverter.hpp: nothing of it is used.
#pragma once
#include <grid_map_core/GridMap.hpp>
