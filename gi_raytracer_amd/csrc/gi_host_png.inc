// gi_host_png.inc -- PNG -> RGBA8 as QImage::pixelColor presents it: the decoder behind `imTex` lines and gih_load_png.
// Included by gi_host.cpp (second piece, inside its unnamed namespace); needs <zlib.h>.

// 8-bit, non-interlaced PNGs of colour type 0 (grey), 2 (RGB), 3 (palette, tRNS), 4 (grey + alpha), 6 (RGBA).  QImage converts none of these
// (no gamma / colour management unless asked), so pixelColor() returns the stored channel values; 16-bit and interlaced files are
// refused.  has_alpha = what QImage::hasAlphaChannel() reports: an alpha channel in the file or a tRNS chunk.
inline uint32_t be32(const unsigned char* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]; }
bool decode_png(const std::string& path, int& w, int& h, bool& has_alpha, std::vector<uint8_t>& rgba, std::string& err)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { err = "cannot open image: " + path; return false; }
    std::vector<unsigned char> file;
    unsigned char buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + got);
    fclose(f);
    static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (file.size() < 8 || memcmp(file.data(), sig, 8) != 0) { err = "not a PNG file: " + path; return false; }
    int depth = 0, ctype = 0, interlace = 0;
    std::vector<unsigned char> idat, plte, trns;
    w = h = 0;
    for (size_t pos = 8; pos + 12 <= file.size();) {
        const uint32_t len = be32(&file[pos]);
        const char* type = reinterpret_cast<const char*>(&file[pos + 4]);
        if (pos + 12 + (size_t)len > file.size()) { err = "truncated PNG: " + path; return false; }
        const unsigned char* data = &file[pos + 8];
        if (memcmp(type, "IHDR", 4) == 0 && len >= 13) { w = (int)be32(data); h = (int)be32(data + 4); depth = data[8]; ctype = data[9]; interlace = data[12]; }
        else if (memcmp(type, "PLTE", 4) == 0) plte.assign(data, data + len);
        else if (memcmp(type, "tRNS", 4) == 0) trns.assign(data, data + len);
        else if (memcmp(type, "IDAT", 4) == 0) idat.insert(idat.end(), data, data + len);
        else if (memcmp(type, "IEND", 4) == 0) break;
        pos += 12 + (size_t)len;
    }
    if (w <= 0 || h <= 0 || w > 32768 || h > 32768) { err = "PNG without a usable IHDR: " + path; return false; }
    if (depth != 8 || interlace != 0) { err = "PNG must be 8 bits per channel and not interlaced: " + path; return false; }
    int ch = 0;
    switch (ctype) { case 0: ch = 1; break; case 2: ch = 3; break; case 3: ch = 1; break; case 4: ch = 2; break; case 6: ch = 4; break; default: err = "PNG colour type not supported: " + path; return false; }
    const size_t stride = (size_t)w * ch;
    std::vector<unsigned char> raw((stride + 1) * (size_t)h);
    uLongf raw_len = (uLongf)raw.size();
    if (uncompress(raw.data(), &raw_len, idat.data(), (uLong)idat.size()) != Z_OK || raw_len != raw.size()) { err = "PNG data does not inflate: " + path; return false; }
    std::vector<unsigned char> img(stride * (size_t)h);
    for (int y = 0; y < h; y++) {                       // undo the scanline filters (PNG spec 9.2)
        const unsigned char* in = &raw[(stride + 1) * (size_t)y];
        unsigned char* out = &img[stride * (size_t)y];
        const unsigned char* up = y ? out - stride : nullptr;
        const int ft = in[0];
        for (size_t x = 0; x < stride; x++) {
            const int a = x >= (size_t)ch ? out[x - ch] : 0, b = up ? up[x] : 0, c = (up && x >= (size_t)ch) ? up[x - ch] : 0;
            int pred = 0;
            if (ft == 1) pred = a;
            else if (ft == 2) pred = b;
            else if (ft == 3) pred = (a + b) >> 1;
            else if (ft == 4) { const int pp = a + b - c, pa = abs(pp - a), pb = abs(pp - b), pc = abs(pp - c); pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c); }
            else if (ft != 0) { err = "PNG filter type out of range: " + path; return false; }
            out[x] = (unsigned char)(in[1 + x] + pred);
        }
    }
    has_alpha = ctype == 4 || ctype == 6 || !trns.empty();
    rgba.resize((size_t)w * h * 4);
    for (size_t i = 0; i < (size_t)w * h; i++) {
        unsigned char r = 0, g = 0, b = 0, a = 255;
        const unsigned char* px = &img[i * ch];
        if (ctype == 0) { r = g = b = px[0]; if (trns.size() >= 2 && px[0] == trns[1]) a = 0; }
        else if (ctype == 2) { r = px[0]; g = px[1]; b = px[2]; if (trns.size() >= 6 && r == trns[1] && g == trns[3] && b == trns[5]) a = 0; }
        else if (ctype == 3) { const size_t k = px[0]; if (k * 3 + 2 < plte.size()) { r = plte[k * 3]; g = plte[k * 3 + 1]; b = plte[k * 3 + 2]; } if (k < trns.size()) a = trns[k]; }
        else if (ctype == 4) { r = g = b = px[0]; a = px[1]; }
        else { r = px[0]; g = px[1]; b = px[2]; a = px[3]; }
        rgba[i * 4] = r; rgba[i * 4 + 1] = g; rgba[i * 4 + 2] = b; rgba[i * 4 + 3] = a;
    }
    return true;
}
