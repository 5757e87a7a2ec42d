// watershedgridtoshp -w <wfile> -poly <layer> [-rings host|device] [--gpus N]   (the toolbox step "Watershed Grid To Shapefile": pyfiles/WatershedGridToShapefile.py takes the
// watershed grid and the output shapefile as its two arguments)
#include "cli_common.hpp"

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    std::string wfile, polyfile, rings = "host";
    bool ok = argc > 2;
    int i = 1;
    while (ok && argc > i) {
        std::string* dst = strcmp(argv[i], "-w") == 0 ? &wfile : strcmp(argv[i], "-poly") == 0 ? &polyfile : strcmp(argv[i], "-rings") == 0 ? &rings : nullptr;
        i++;
        if (!dst || argc <= i) ok = false;
        else *dst = argv[i++];
    }
    if (!ok || wfile.empty() || polyfile.empty()) {
        printf("Usage: %s -w <watershed grid> -poly <polygon layer: .shp, .json or .geojson> [-rings host|device] [--gpus N]\n", argv[0]);
        printf("  -rings: where the rings are closed: host (the default) or device; both write the same bytes\n");
        return 0;
    }
    if (rings != "host" && rings != "device") {   // refused before anything is read
        fprintf(stderr, "watershedgridtoshp: -rings %s: host or device\n", rings.c_str());
        return 2;
    }
    tdx_tool_set_polygon_rings(rings == "device" ? 1 : 0);
    const int err = tdx_tool_watershedgridtoshp(wfile.c_str(), polyfile.c_str());
    if (err == TDX_ERR_ARG) return 2;   // an output this build cannot write: said on stderr
    return cli::finish("WatershedGridToShapefile", err);
}
