// fid_map.hip -- the map of fiducials a context poses the camera against (fid_abi.h: "one camera pose per frame from a map of
// fiducials").  Part of the fid_api.hip translation unit; host code, no device.
//
// The file is the one fiducial_slam keeps (fiducial_slam/src/map.cpp:541-625): a line per fiducial,
//     id x y z roll pitch yaw variance numObs [links ...]
// with the angles in degrees.  A line counts when its first nine fields read as int, 7 x double, int (whatever follows them is the
// link list, which a pose does not need); any other line is passed over and counted, as the reference warns and carries on.
#include <stdio.h>

namespace {

thread_local std::string g_map_error;

// tf2::Quaternion::setRPY(roll, pitch, yaw) as a matrix: Rz(yaw) Ry(pitch) Rx(roll)
void map_rpy_matrix(double roll, double pitch, double yaw, double R[9])
{
    const double cr = cos(roll), sr = sin(roll), cp = cos(pitch), sp = sin(pitch), cy = cos(yaw), sy = sin(yaw);
    R[0] = cy * cp; R[1] = cy * sp * sr - sy * cr; R[2] = cy * sp * cr + sy * sr;
    R[3] = sy * cp; R[4] = sy * sp * sr + cy * cr; R[5] = sy * sp * cr - cy * sr;
    R[6] = -sp;     R[7] = cp * sr;                R[8] = cp * cr;
}

void map_fill_entry(int32_t id, double len, const double xyz[3], const double rpy_deg[3], fid_map_entry *e)
{
    const double d2r = 3.14159265358979323846 / 180.0;
    e->id = id;
    e->reserved0 = 0;
    e->len = len;
    map_rpy_matrix(rpy_deg[0] * d2r, rpy_deg[1] * d2r, rpy_deg[2] * d2r, e->R);
    for (int i = 0; i < 3; i++) e->t[i] = xyz[i];
}

}  // namespace

const char *fid_map_last_error(void) { return g_map_error.c_str(); }

fid_status fid_map_entry_from_rpy(int32_t id, double len, const double xyz[3], const double rpy_deg[3], fid_map_entry *out)
{
    g_map_error.clear();
    if (!xyz || !rpy_deg || !out) return FID_E_INVALID_ARG;
    if (!(len > 0)) {
        g_map_error = "len must be positive";
        return FID_E_INVALID_ARG;
    }
    map_fill_entry(id, len, xyz, rpy_deg, out);
    return FID_OK;
}

fid_status fid_map_load_file(const char *path, double fiducial_len, fid_map_entry *entries, int32_t cap, int32_t *n, int32_t *n_skipped)
{
    g_map_error.clear();
    if (n) *n = 0;
    if (n_skipped) *n_skipped = 0;
    if (!path || !n || cap < 0 || (cap > 0 && !entries)) return FID_E_INVALID_ARG;
    if (!(fiducial_len > 0)) {
        g_map_error = "fiducial_len must be positive";
        return FID_E_INVALID_ARG;
    }
    FILE *fp = fopen(path, "r");
    if (!fp) {
        g_map_error = std::string("cannot open ") + path;
        return FID_E_INVALID_ARG;
    }
    std::vector<fid_map_entry> got;
    int skipped = 0, lineno = 0;
    std::string line;
    fid_status rc = FID_OK;
    for (;;) {
        // a whole line, however long its link list is
        line.clear();
        int ch;
        while ((ch = fgetc(fp)) != EOF && ch != '\n') line.push_back((char)ch);
        if (ch == EOF && line.empty()) break;
        lineno++;
        int id = 0, num_obs = 0;
        double v[7];
        const int fields = sscanf(line.c_str(), "%d %lf %lf %lf %lf %lf %lf %lf %d", &id, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &num_obs);
        if (fields != 9) {
            skipped++;
            continue;
        }
        bool twice = false;
        for (const fid_map_entry &e : got) twice = twice || e.id == id;
        if (twice) {
            g_map_error = "line " + std::to_string(lineno) + ": id " + std::to_string(id) + " appears twice";
            rc = FID_E_INVALID_ARG;
            break;
        }
        fid_map_entry e;
        map_fill_entry(id, fiducial_len, v, v + 3, &e);
        got.push_back(e);
    }
    fclose(fp);
    if (n_skipped) *n_skipped = skipped;
    if (rc != FID_OK) return rc;
    *n = (int32_t)got.size();
    if ((int64_t)got.size() > cap) {
        g_map_error = "the file holds " + std::to_string(got.size()) + " entries, the caller has room for " + std::to_string(cap);
        return FID_E_CAPACITY;
    }
    for (size_t i = 0; i < got.size(); i++) entries[i] = got[i];
    return FID_OK;
}
