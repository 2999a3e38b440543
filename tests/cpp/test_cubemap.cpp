// tests/cpp/test_cubemap.cpp -- RayTracer::bakeReflectionProbe (an addition to the drop-in class) on a loaded scene: argv[1] = .scn, argv[2 .. 4] = the
// probe's position, argv[5] = face, argv[6] = samples, argv[7] = levels.  Prints the sizes of the levels and, per level, the sum of its values added
// one by one from 0 with all digits, for the test to compare with the Python mirror's; then what bad arguments do.
#include <cstdio>
#include <cstdlib>
#include "../../include/gi/builtin_loaders.h"

int main(int argc, char** argv)
{
    if (argc < 8) return 2;
    const gi::dvec3 pos(strtod(argv[2], nullptr), strtod(argv[3], nullptr), strtod(argv[4], nullptr));
    const int face = atoi(argv[5]), samples = atoi(argv[6]), levels = atoi(argv[7]);
    Camera camera(gi::dvec3(10, 5, 0), gi::dvec3(0, 0, 0));
    RayTracer raytracer(camera);
    Octree* scene = new Octree();
    loadScene(scene, raytracer, argv[1]);
    raytracer.setScene(scene);
    scene->rebuild();
    std::vector<std::vector<double>> chain;
    if (!raytracer.bakeReflectionProbe(pos, face, samples, chain, levels)) { printf("failed: %s\n", raytracer.last_error().c_str()); return 1; }
    printf("levels %zu\n", chain.size());
    for (size_t l = 0; l < chain.size(); l++) {
        double sum = 0;
        for (double v : chain[l]) sum += v;
        printf("level %zu size %zu sum %.17g\n", l, chain[l].size(), sum);
    }
    const size_t kept = chain.size();
    const bool refused = !raytracer.bakeReflectionProbe(pos, 0, samples, chain) && !raytracer.bakeReflectionProbe(pos, face, 0, chain) &&
                         !raytracer.bakeReflectionProbe(pos, 6, samples, chain, 3) && !raytracer.bakeReflectionProbe(pos, face, samples, chain, 13);
    printf("bad arguments refused %d kept %d\n", (int)refused, (int)(chain.size() == kept));
    return 0;
}
