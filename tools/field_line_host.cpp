// field_line_host.cpp -- xpic_amd/csrc/field_line_step.h compiled for the host and run on an analytic field, so that
// tests/test_field_line_host.py can hold the header's own text to the numpy restatement (tests/field_lines_ref.py) bit for
// bit without a GPU, as tools/full_orbit_host.cpp does for the full-orbit steps.  A stand-alone program: it reads its seeds
// from the command line and prints one line per lane.
//   field_line_host <h> <max_steps> <f_floor> <close_tol> <zmax> <launch_steps> x y z [x y z ...]
// The field is F = (-(y - 2), x - 2, 0.3 + 0.1 z), written so that numpy forms the same operations; the region keeps
// z < zmax.  Output per seed and direction: end x y z, length, volume, fmin, smin, fmax as hexadecimal floats, steps, code.
// Build: c++ -O2 -std=c++17 -ffp-contract=off tools/field_line_host.cpp -o field_line_host
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../xpic_amd/csrc/field_line_step.h"

struct Source {
  void at(const double* r, double* F) const
  {
    F[0] = -(r[1] - 2.0);
    F[1] = r[0] - 2.0;
    F[2] = 0.3 + 0.1 * r[2];
  }
};

int main(int argc, char** argv)
{
  if (argc < 10 || (argc - 7) % 3 != 0) {
    std::fprintf(stderr, "usage: field_line_host h max_steps f_floor close_tol zmax launch_steps x y z [x y z ...]\n");
    return 2;
  }
  const double h = std::atof(argv[1]), f_floor = std::atof(argv[3]), close_tol = std::atof(argv[4]), zmax = std::atof(argv[5]);
  const long long max_steps = std::atoll(argv[2]);
  const int launch_steps = std::atoi(argv[6]);
  const Source src;
  for (int a = 7; a + 2 < argc; a += 3) {
    const double seed[3] = {std::atof(argv[a]), std::atof(argv[a + 1]), std::atof(argv[a + 2])};
    for (int dir = 0; dir < 2; ++dir) {
      xpic::FLState L{{seed[0], seed[1], seed[2]}, 0.0, 0.0, std::numeric_limits<double>::infinity(), 0.0, 0.0, 0};
      int code = XPIC_LINE_RUNNING;
      while (code == XPIC_LINE_RUNNING) // launches, as the device's host loop makes them
        code = xpic::fl_advance(src, [&](const double* r) { return r[2] < zmax; }, [](const xpic::FLState&) {},
          dir ? -1.0 : 1.0, h, f_floor, close_tol, max_steps, launch_steps, seed, L);
      std::printf("%a %a %a %a %a %a %a %a %lld %d\n", L.r[0], L.r[1], L.r[2], L.length, L.volume, L.fmin, L.smin, L.fmax,
        L.steps, code);
    }
  }
  return 0;
}
