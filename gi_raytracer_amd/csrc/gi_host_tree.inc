// gi_host_tree.inc -- the pre-order octree tables and the one partition that fills them, with the reference's two rules (scene entities,
// photons).  Included by gi_host.cpp (third piece, after gi_host_geom.inc).

const int kMaxEntitiesPerLeaf = 16;    // include/util.h:14
const int kMaxPhotonsPerLeaf = 16;     // include/util.h:15
const double kMinLeafSize = .0015;     // include/util.h:16
const double kMaxSubdivRatio = 0.75;   // include/util.h:17

// Nodes in pre-order: 6 box values and 8 children (-1 = none) per node; node i lists idx[off[i] .. off[i + 1]), which is empty for an inner node.
struct OctreeTables {
    std::vector<double> bbox;
    std::vector<int32_t> child, off, idx;
    void clear() { bbox.clear(); child.clear(); off.clear(); idx.clear(); }
    int n_nodes() const { return (int)(bbox.size() / 6); }
    int new_node(const Aabb& b)
    {
        const int id = n_nodes();
        bbox.resize(bbox.size() + 6);
        store_box(b, &bbox[(size_t)id * 6]);
        child.insert(child.end(), 8, -1);
        off.push_back((int32_t)idx.size());   // start; the end is the next node's start
        return id;
    }
    void close() { off.push_back((int32_t)idx.size()); }
};

// Octree::Node::partition and PhotonMap::Node::partition as one emitter of pre-order tables: fills node `id` (already created, box `cell`)
// holding `items`; `split` says whether it is partitioned.  A child is created and linked right before its own subtree is emitted.
template <class Rule>
void partition(OctreeTables& t, int id, const Aabb& cell, const std::vector<int>& items, bool split, const Rule& rule)
{
    if (!split) { t.idx.insert(t.idx.end(), items.begin(), items.end()); return; }   // leaf: owns its items
    Aabb oc[8];
    octants(cell, oc);
    std::vector<int> part[8];
    for (int it : items)
        for (int i = 0; i < 8; i++)
            if (rule.holds(it, oc[i])) part[i].push_back(it);
    double mean = 0;
    for (int i = 0; i < 8; i++) mean += (double)part[i].size();
    mean /= 8;
    const bool frozen = mean > kMaxSubdivRatio * (double)items.size();   // "skipped" subdivision: children stay leaves
    for (int i = 0; i < 8; i++) {
        if (part[i].empty() && !Rule::kEmptyChildren) continue;
        const int ch = t.new_node(oc[i]);
        t.child[(size_t)id * 8 + i] = ch;
        partition(t, ch, oc[i], part[i], !frozen && rule.again((int)part[i].size(), oc[i]), rule);
    }
}

// A whole tree over items 0 .. n-1 in the box `root`; the root splits when it holds more than the rule's leaf limit.
template <class Rule>
void build_tree(OctreeTables& t, const Aabb& root, int n, const Rule& rule)
{
    t.clear();
    std::vector<int> all((size_t)n);
    for (int i = 0; i < n; i++) all[i] = i;
    partition(t, t.new_node(root), root, all, n > Rule::kMaxPerLeaf, rule);
    t.close();
}

// Octree::Node::partition, include/octree.cpp:316-384: an entity goes where its box and its own cell test agree, flat entities nowhere;
// empty children are null; a child splits again above 16 entities while it is wider than the leaf-size floor.  Store is Entities
// (gi_host_scene.inc), named by the caller because that piece comes after this one.
template <class Store>
struct EntityRule {
    static const bool kEmptyChildren = false;
    static const int kMaxPerLeaf = kMaxEntitiesPerLeaf;
    const Store& ent;
    bool holds(int e, const Aabb& oc) const { return closed_overlap(oc, ent.box[e]) && ent.in_cell(e, oc) && ext_x(ent.box[e]) > kEps; }
    bool again(int n, const Aabb& oc) const { return n > kMaxPerLeaf && ext_x(oc) > kMinLeafSize; }
};

// PhotonMap::Node::partition, include/photonMap.cpp:137-192: a photon goes where its origin lies half-open; all eight children always
// exist; a child splits again above 16 photons.  As there, a photon that no octant holds (above the upper corners' mid + .5*extent, or more
// than 16 within a few rounding steps of each other, once their cell is that small) is listed by no leaf.
struct PhotonRule {
    static const bool kEmptyChildren = true;
    static const int kMaxPerLeaf = kMaxPhotonsPerLeaf;
    const double* photons;   // 9 values per photon, the origin first
    bool holds(int p, const Aabb& oc) const { return half_open_contains(oc, d3(photons + (size_t)p * 9)); }
    bool again(int n, const Aabb&) const { return n > kMaxPerLeaf; }
};
