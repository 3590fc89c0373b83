/* tables_driver.cpp -- SceneTablesInRange (tracerboy_amd/csrc/host/lds_image.h) on the tables of a two-triangle scene built by hand, sound and then
 * with one thing broken at a time (tests/test_scene_tables.py reads the lines: NAME 0|1).  The tables are vectors of exactly their size, so that a
 * check that read past one would be the sanitizer's finding. */
#include "lds_image.h"
#include <cstdio>
#include <vector>

struct Tables {
    std::vector<TbTriB> tris; std::vector<TbDevHitGroup> hitGroups; std::vector<uint32_t> indices; size_t numVertexFloats, numMaterials;
    bool inRange() const
    {
        return SceneTablesInRange(tris.data(), tris.size(), hitGroups.data(), hitGroups.size(), indices.data(), indices.size(), numVertexFloats, numMaterials);
    }
};

static Tables quad() /* one geometry, one material: four vertices of 8 floats, two triangles over them */
{
    Tables t;
    t.tris.resize(2);
    for (uint32_t p = 0; p < 2; p++) { t.tris[p] = TbTriB{}; t.tris[p].geometryIndex = 0; t.tris[p].primitiveIndex = p; t.tris[p].geometryFlags = 1; }
    t.hitGroups = {TbDevHitGroup{0, 0, 0, 0}};
    t.indices = {0, 1, 2, 0, 2, 3};
    t.numVertexFloats = 4 * 8; t.numMaterials = 1;
    return t;
}

int main()
{
    Tables t = quad();
    printf("sound %d\n", t.inRange());
    t = quad(); t.tris[1].geometryIndex = 1;           /* one past the last hit group */
    printf("geometry_index_past_the_end %d\n", t.inRange());
    t = quad(); t.hitGroups[0].iFirst = 1;             /* primitive 1's triple: indices 4, 5 and 6 of 6 */
    printf("triple_straddles_the_end %d\n", t.inRange());
    t = quad(); t.hitGroups[0].vFirst = 1;             /* vertex 3's last float: float 32 of 32 */
    printf("vertex_last_float_past_the_end %d\n", t.inRange());
    t = quad(); t.hitGroups[0].MaterialIndex = 1;      /* the count itself */
    printf("material_index_is_the_count %d\n", t.inRange());
    t = quad(); t.indices[5] = 0x20000003u;            /* 8 * index = 2^32 + 24: in 32 bits vertex 3 */
    printf("vertex_index_wraps_in_32_bits %d\n", t.inRange());
    t = quad(); t.tris[1].primitiveIndex = 0x55555556u; /* 3 * primitive = 2^32 + 2: in 32 bits a triple inside the table */
    printf("primitive_index_wraps_in_32_bits %d\n", t.inRange());
    t = quad(); t.tris.clear();                        /* no triangle: nothing to form an index from */
    printf("no_triangles %d\n", t.inRange());
    return 0;
}
