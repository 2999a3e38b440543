// tests/cpp/test_lens.cpp -- RayTracer::setLens and RayTracer::focusAt (additions to the drop-in class) on a loaded scene: argv[1] = .scn,
// argv[2] = width, argv[3] = height.  Prints the sum of the first-hit depth buffer (2 samples) under a lens, through the pinhole, and under the
// lens refocused, with all digits, for the test to compare with the Python mirror's.
#include <cstdio>
#include <cstdlib>
#include "../../include/gi/builtin_loaders.h"

static double depth_sum(RayTracer& rt, int w, int h)
{
    RayTracer::Features f;
    if (!rt.renderFeatures(w, h, 2, f)) { printf("failed: %s\n", rt.last_error().c_str()); exit(1); }
    double d = 0;
    for (double v : f.depth) d += v;
    return d;
}

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    const int w = atoi(argv[2]), h = atoi(argv[3]);
    Camera camera(gi::dvec3(10, 5, 0), gi::dvec3(0, 0, 0));
    RayTracer raytracer(camera);
    Octree* scene = new Octree();
    loadScene(scene, raytracer, argv[1]);
    raytracer.setScene(scene);
    scene->rebuild();
    const double pinhole = depth_sum(raytracer, w, h);
    if (!raytracer.setLens(0.25, 7, 0.5)) { printf("failed: %s\n", raytracer.last_error().c_str()); return 1; }
    const double lens = depth_sum(raytracer, w, h);
    const bool refused = !raytracer.setLens(-1.0) && !raytracer.setLens(0.25, 2) && !raytracer.setLens(0.25, 17) && !raytracer.focusAt(0.0) && !raytracer.focusAt(-3.0);
    printf("bad lens refused %d\n", (int)refused);
    printf("lens kept %d\n", (int)(depth_sum(raytracer, w, h) == lens));
    if (!raytracer.focusAt(6.0)) return 1;
    const double focused = depth_sum(raytracer, w, h);
    printf("lens sum %.17g pinhole sum %.17g focused sum %.17g\n", lens, pinhole, focused);
    return 0;
}
