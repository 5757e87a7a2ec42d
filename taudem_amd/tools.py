"""File-level tool functions with the names and argument lists of the reference's tool functions
(the interface the reference's ``*mn.cpp`` mains and the ArcGIS ``pyfiles/*.py`` wrappers drive):

    flood      src/flood.h:1-2            setdird8  src/d8.h:5          aread8  src/aread8.h:3
    setdir     src/dinf.cpp:109           area      src/areadinf.h:2    dmarea  src/dinfdecayaccum.cpp:61-62

They read GeoTIFF inputs, run the HIP hot path on one GPU and write GeoTIFF outputs; return codes are
the reference's (0 ok, 1 mismatch; 21/22/5 where the reference would MPI_Abort with that code).
"""
from __future__ import annotations

from . import _lib


def _b(s):
    return (s or "").encode()


def set_device(device: int):
    return _lib.load().tdx_tool_set_device(int(device))


def flood(demfile, felfile, sfdrfile="", usesfdr=0, verbose=False, is_4Point=False, use_mask=False, maskfile=""):
    return _lib.load().tdx_tool_pitremove(_b(demfile), _b(felfile), _b(sfdrfile), int(usesfdr), int(verbose), int(is_4Point), int(use_mask), _b(maskfile))


def setdird8(demfile, pointfile, slopefile, flowfile="", useflowfile=0):
    return _lib.load().tdx_tool_d8flowdir(_b(demfile), _b(pointfile), _b(slopefile), _b(flowfile), int(useflowfile))


def aread8(pfile, afile, datasrc="", lyrname="", uselyrname=0, lyrno=0, wfile="", useOutlets=0, usew=0, contcheck=1):
    return _lib.load().tdx_tool_aread8(_b(pfile), _b(afile), _b(datasrc), _b(lyrname), int(uselyrname), int(lyrno), _b(wfile), int(useOutlets),
                                      int(usew), int(contcheck))


def setdir(demfile, angfile, slopefile, flowfile="", useflowfile=0):
    return _lib.load().tdx_tool_dinfflowdir(_b(demfile), _b(angfile), _b(slopefile), _b(flowfile), int(useflowfile))


def area(angfile, scafile, datasrc="", lyrname="", uselyrname=0, lyrno=0, wfile="", useOutlets=0, usew=0, contcheck=1):
    return _lib.load().tdx_tool_areadinf(_b(angfile), _b(scafile), _b(datasrc), _b(lyrname), int(uselyrname), int(lyrno), _b(wfile),
                                        int(useOutlets), int(usew), int(contcheck))


def dmarea(angfile, adecfile, dmfile, datasrc="", lyrname="", uselyrname=0, lyrno=0, wfile="", useOutlets=0, usew=0, contcheck=1):
    return _lib.load().tdx_tool_dinfdecayaccum(_b(angfile), _b(adecfile), _b(dmfile), _b(datasrc), _b(lyrname), int(uselyrname), int(lyrno),
                                              _b(wfile), int(useOutlets), int(usew), int(contcheck))


def gridnet(pfile, plenfile, tlenfile, gordfile, maskfile="", datasrc="", lyrname="", uselyrname=0, lyrno=0, useMask=0, useOutlets=0, thresh=0):
    return _lib.load().tdx_tool_gridnet(_b(pfile), _b(plenfile), _b(tlenfile), _b(gordfile), _b(maskfile), _b(datasrc), _b(lyrname), int(uselyrname),
                                       int(lyrno), int(useMask), int(useOutlets), int(thresh))


def d8flowpathextremeup(pfile, safile, ssafile, usemax=1, datasrc="", lyrname="", uselyrname=0, lyrno=0, useOutlets=0, contcheck=1):
    return _lib.load().tdx_tool_d8flowpathextremeup(_b(pfile), _b(safile), _b(ssafile), int(usemax), _b(datasrc), _b(lyrname), int(uselyrname), int(lyrno),
                                                   int(useOutlets), int(contcheck))


def threshold(ssafile, srcfile, maskfile="", thresh=100.0, usemask=0):
    return _lib.load().tdx_tool_threshold(_b(ssafile), _b(srcfile), _b(maskfile), float(thresh), int(usemask))


def nameadd(arg: str, suff: str) -> str:
    """nameadd() of src/commonLib.cpp:53-73: insert `suff` before the extension of `arg`."""
    dot = arg.rfind(".")
    if dot < 0:
        return arg + suff
    ext = arg[dot:]
    return arg[:dot] + suff + ("" if "." in suff else ext)


def depgrd(angfile, dgfile, depfile):
    """src/DinfUpDependence.cpp:52"""
    return _lib.load().tdx_tool_dinfupdependence(_b(angfile), _b(dgfile), _b(depfile))


def dsaccum(angfile, wgfile, raccfile, dmaxfile):
    """src/DinfRevAccum.cpp:51"""
    return _lib.load().tdx_tool_dinfrevaccum(_b(angfile), _b(wgfile), _b(raccfile), _b(dmaxfile))


def dinfdistdown(angfile, felfile, slpfile, wfile, srcfile, dtsfile, statmethod=0, typemethod=0, usew=0, concheck=1):
    """src/DinfDistDown.cpp:66"""
    return _lib.load().tdx_tool_dinfdistdown(_b(angfile), _b(felfile), _b(slpfile), _b(wfile), _b(srcfile), _b(dtsfile), int(statmethod), int(typemethod),
                                             int(usew), int(concheck))


def dinfdistup(angfile, felfile, slpfile, wfile, rtrfile, statmethod=0, typemethod=0, usew=0, concheck=1, thresh=0.0):
    """src/DinfDistUp.cpp:65"""
    return _lib.load().tdx_tool_dinfdistup(_b(angfile), _b(felfile), _b(slpfile), _b(wfile), _b(rtrfile), int(statmethod), int(typemethod), int(usew),
                                           int(concheck), float(thresh))


def retlimro(angfile, wgfile, rcfile, qrlfile):
    """src/RetlimFlow.cpp:53 (RetLimFlow)"""
    return _lib.load().tdx_tool_retlimflow(_b(angfile), _b(wgfile), _b(rcfile), _b(qrlfile))


def avalancherunoutgrd(angfile, felfile, assfile, rzfile, dmfile, thresh=0.2, alpha=18.0, path=1):
    """src/DinfAvalanche.cpp:62 (DinfAvalanche)"""
    return _lib.load().tdx_tool_dinfavalanche(_b(angfile), _b(felfile), _b(assfile), _b(rzfile), _b(dmfile), float(thresh), float(alpha), int(path))


def distgrid(pfile, srcfile, distfile, thresh=1):
    """src/D8HDistToStrm.cpp:57 (D8HDistToStrm)"""
    return _lib.load().tdx_tool_d8hdisttostrm(_b(pfile), _b(srcfile), _b(distfile), int(thresh))


d8hdisttostrm = distgrid


def gagewatershed(pfile, wfile, datasrc, lyrname="", uselyrname=0, lyrno=0, idfile="", writeid=0, writeupid=0, upidfile=""):
    """src/gagewatershed.cpp:56 (writeupid = 1 is refused)"""
    return _lib.load().tdx_tool_gagewatershed(_b(pfile), _b(wfile), _b(datasrc), _b(lyrname), int(uselyrname), int(lyrno), _b(idfile), int(writeid),
                                              int(writeupid), _b(upidfile))


def flowdircond(pfile, zfile, zfdcfile):
    """src/flowdircond.cpp:54 (FlowDirCond)"""
    return _lib.load().tdx_tool_flowdircond(_b(pfile), _b(zfile), _b(zfdcfile))


def d8vdistdown(pfile, felfile, srcfile, distfile, thresh=1):
    """src/D8VDistToStrm.cpp:58 (D8VDistToStrm)"""
    return _lib.load().tdx_tool_d8vdisttostrm(_b(pfile), _b(felfile), _b(srcfile), _b(distfile), int(thresh))


d8vdisttostrm = d8vdistdown


def sloped(pfile, felfile, slpdfile, dn=50.0):
    """src/SlopeAveDown.cpp:59 (SlopeAveDown; a dn that is negative or not finite is refused)"""
    return _lib.load().tdx_tool_slopeavedown(_b(pfile), _b(felfile), _b(slpdfile), float(dn))


slopeavedown = sloped


def catchhydrogeo(handfile, catchfile, catchlistfile, slpfile, hfile, hpfile):
    """src/CatchHydroGeo.cpp:69 (CatchHydroGeo)"""
    return _lib.load().tdx_tool_catchhydrogeo(_b(handfile), _b(catchfile), _b(catchlistfile), _b(slpfile), _b(hfile), _b(hpfile))


def inundepth(handfile, catchfile, maskfile, fcfile, hpfile, mapfile, depthfile=None):
    """src/InunDepth.cpp:53 (InunDepth); maskfile / depthfile None or "": not given.  With a mask the map is nodata everywhere, as in the reference."""
    return _lib.load().tdx_tool_inundepth(_b(handfile), _b(catchfile), _b(maskfile) if maskfile else None, _b(fcfile), _b(hpfile), _b(mapfile),
                                          _b(depthfile) if depthfile else None)


def dropan(areafile, dirfile, elevfile, ssafile, dropfile, datasrc, lyrname="", uselyrname=0, lyrno=0, threshmin=5.0, threshmax=500.0, nthresh=10, steptype=0):
    """src/DropAnalysis.cpp:172 (DropAnalysis): writes the table dropfile; returns (code, optimum threshold - 0.0 when no threshold qualifies)."""
    import ctypes

    opt = ctypes.c_float(0.0)
    rc = _lib.load().tdx_tool_dropanalysis(_b(areafile), _b(dirfile), _b(elevfile), _b(ssafile), _b(dropfile), _b(datasrc), _b(lyrname), int(uselyrname), int(lyrno),
                                           float(threshmin), float(threshmax), int(nthresh), int(steptype), ctypes.byref(opt))
    return rc, float(opt.value)


dropanalysis = dropan


def peukerdouglas(felfile, ssfile, p=(0.4, 0.1, 0.05)):
    """src/PeukerDouglas.cpp:54 (PeukerDouglas): p = the weights of the centre, the side and the diagonal cells of the smoothing."""
    import ctypes

    w = (ctypes.c_float * 3)(float(p[0]), float(p[1]), float(p[2]))
    return _lib.load().tdx_tool_peukerdouglas(_b(felfile), _b(ssfile), ctypes.cast(w, ctypes.c_void_p))


def sindexcombined(slopefile, scaterrainfile, scarminroadfile, scarmaxroadfile, tergridfile, terparfile, satfile, sincombinedfile, Rminter, Rmaxter, par=(9.81, 1000.0)):
    """src/SinmapSI.cpp:138 (SinmapSI): par = (g, rhow); an empty road file name means that raster is absent.  The four numbers are rounded to float32
    first, as the reference's main scans them."""
    import ctypes

    import numpy as np

    p = (ctypes.c_double * 2)(float(np.float32(par[0])), float(np.float32(par[1])))
    return _lib.load().tdx_tool_sinmapsi(_b(slopefile), _b(scaterrainfile), _b(scarminroadfile or ""), _b(scarmaxroadfile or ""), _b(tergridfile), _b(terparfile),
                                         _b(satfile), _b(sincombinedfile), float(np.float32(Rminter)), float(np.float32(Rmaxter)), ctypes.cast(p, ctypes.c_void_p))


def sinmapsi(slpfile, scafile, calfile, calparfile, sifile, satfile, rminter, rmaxter, g=9.81, rhow=1000.0, scaminfile="", scamaxfile=""):
    """SinmapSI with the arguments in the order of the reference's command line."""
    return sindexcombined(slpfile, scafile, scaminfile, scamaxfile, calfile, calparfile, satfile, sifile, rminter, rmaxter, (g, rhow))


def _two_floats(p):
    import ctypes

    v = (ctypes.c_float * 2)(float(p[0]), float(p[1]))
    return v, ctypes.cast(v, ctypes.c_void_p)


def twigrid(slopefile, areafile, twifile):
    """src/TWI.cpp:49 (TWI)."""
    return _lib.load().tdx_tool_twi(_b(slopefile), _b(areafile), _b(twifile))


def slopearea(slopefile, scafile, safile, p=(2.0, 1.0)):
    """src/SlopeArea.cpp:52 (SlopeArea): p = (m, n), the exponents of slope and area."""
    keep, ptr = _two_floats(p)
    return _lib.load().tdx_tool_slopearea(_b(slopefile), _b(scafile), _b(safile), ptr)


def atanbgrid(slopefile, areafile, atanbfile):
    """src/SlopeAreaRatio.cpp:49 (SlopeAreaRatio)."""
    return _lib.load().tdx_tool_slopearearatio(_b(slopefile), _b(areafile), _b(atanbfile))


def lengtharea(plenfile, ad8file, ssfile, p=(0.03, 1.3)):
    """src/LengthArea.cpp:51 (LengthArea): p = (M, y)."""
    keep, ptr = _two_floats(p)
    return _lib.load().tdx_tool_lengtharea(_b(plenfile), _b(ad8file), _b(ssfile), ptr)


def setregion(fdrfile, regiongwfile, newfile, regionID=1):
    """src/SetRegion.cpp:78 (SetRegion)."""
    return _lib.load().tdx_tool_setregion(_b(fdrfile), _b(regiongwfile), _b(newfile), int(regionID))


def editraster(rasterfile, newfile, changefile):
    """src/EditRaster.cpp:69 (EditRaster): the raster as int16 with the cells of the change file's "x,y,value" lines set."""
    return _lib.load().tdx_tool_editraster(_b(rasterfile), _b(newfile), _b(changefile))


def catchoutlets(pfile, streamnetsrc="", outletsdatasrc="", mindist=0.0, gwstartno=1, minarea=0.0, treefile="", coordfile=""):
    """src/CatchOutlets.cpp:126 (CatchOutlets), host code: the network is the line layer streamnetsrc, or this project's streamnet -tree and -coord files
    (treefile, coordfile) - one of the two.  The outlets go to a shapefile or GeoJSON point layer."""
    return _lib.load().tdx_tool_catchoutlets(_b(pfile), _b(streamnetsrc), _b(treefile), _b(coordfile), _b(outletsdatasrc), float(mindist), int(gwstartno), float(minarea))


def watershedgridtoshp(wfile, polyfile):
    """pyfiles/WatershedGridToShapefile.py (the toolbox step Watershed Grid To Shapefile): the polygons of the watershed grid wfile (read as int32) as a
    shapefile (.shp) or GeoJSON (.json / .geojson) polygon layer with the fields gridcode and cells; any other output is refused before anything is read."""
    return _lib.load().tdx_tool_watershedgridtoshp(_b(wfile), _b(polyfile))


def set_polygon_rings(rings="host"):
    """Where watershedgridtoshp closes the rings from now on: "host" (the default) or "device" (tdx_tool_set_polygon_rings); both write the same bytes."""
    if rings not in _lib.POLYGONIZE_RINGS:
        raise ValueError(f"rings: {rings!r} is neither 'host' nor 'device'")
    return _lib.load().tdx_tool_set_polygon_rings(_lib.POLYGONIZE_RINGS.index(rings))


def siregiontool(dem, parreg, att, parreg_in="", shp="", shp_att_name="ID", att_tmin=2.708, att_tmax=2.708, att_cmin=0.0, att_cmax=0.25, att_phimin=30.0,
                 att_phimax=45.0, att_soildens=2000.0):
    """pyfiles/SIRegionTool.py (the toolbox step Create Parameter Region Grid): the calibration region grid parreg (int16 GeoTIFF, nodata 0) on the grid
    of dem - the polygon layer shp burned in by the field shp_att_name, the region grid parreg_in resampled by nearest neighbour, or one region - and the
    region table att with one line per id that occurs, the seven parameters written as repr(float(value)).  Both sources, an output directory that does
    not exist and a polygon source without a reader are refused before anything is read."""
    import ctypes as C

    texts = [repr(float(v)).encode() for v in (att_tmin, att_tmax, att_cmin, att_cmax, att_phimin, att_phimax, att_soildens)]
    arr = (C.c_char_p * 7)(*texts)
    return _lib.load().tdx_tool_siregiontool(_b(dem), _b(parreg), _b(att), _b(parreg_in), _b(shp), _b(shp_att_name), C.cast(arr, C.c_void_p))


twi = twigrid
slopearearatio = atanbgrid


def netsetup(pfile, srcfile, ordfile, ad8file, elevfile, treefile, coordfile, outletsds="", lyrname="", uselayername=0, lyrno=0, wfile="", streamnetsrc="",
             streamnetlyr="", useOutlets=0, ordert=1, verbose=False):
    """src/streamnet.cpp:372 (StreamNet); ordert = 0 is -sw.  The stream network layer is not written: a non-empty streamnetsrc / streamnetlyr is refused
    (tdx_streamnet_net_write, Context.streamnet(..., net=path), makes the layer from the links)."""
    return _lib.load().tdx_tool_streamnet(_b(pfile), _b(srcfile), _b(ordfile), _b(ad8file), _b(elevfile), _b(treefile), _b(coordfile), _b(outletsds), _b(lyrname),
                                          int(uselayername), int(lyrno), _b(wfile), _b(streamnetsrc), _b(streamnetlyr), int(useOutlets), int(ordert), int(bool(verbose)))


streamnet = netsetup


def set_streamnet_links(links="host"):
    """Where netsetup builds the links from now on: "host" (the default) or "device" (tdx_tool_set_streamnet_links); both write the same bytes."""
    if links not in _lib.STREAMNET_LINKS:
        raise ValueError(f"links: one of {_lib.STREAMNET_LINKS}, not {links!r}")
    return _lib.load().tdx_tool_set_streamnet_links(_lib.STREAMNET_LINKS.index(links))


def outletstosrc(pfile, srcfile, outletsdatasrc, outletslayer="", uselyrname=0, lyrno=0, outletmoveddatasrc="", outletmovedlayer="", maxdist=50):
    """src/MoveOutletsToStrm.cpp:80 (MoveOutletsToStrm).  The moved outlets go to a shapefile (.shp) or GeoJSON (.json / .geojson) layer; any other
    output is refused before anything is read.  The layer arguments are accepted and ignored."""
    return _lib.load().tdx_tool_moveoutletstostrm(_b(pfile), _b(srcfile), _b(outletsdatasrc), _b(outletslayer), int(uselyrname), int(lyrno), _b(outletmoveddatasrc),
                                                  _b(outletmovedlayer), int(maxdist))


moveoutletstostrm = outletstosrc


def connectdown(pfile, wfile, ad8file, outletdatasrc, outletlyr="", movedoutletdatasrc="", movedoutletlyr="", movedist=10):
    """src/ConnectDown.cpp:79 (ConnectDown).  Both outputs are shapefile or GeoJSON point layers, as for outletstosrc."""
    return _lib.load().tdx_tool_connectdown(_b(pfile), _b(wfile), _b(ad8file), _b(outletdatasrc), _b(outletlyr), _b(movedoutletdatasrc), _b(movedoutletlyr), int(movedist))


def dsllArea(angfile, ctptfile, dmfile, datasrc="", lyrname="", uselyrname=0, lyrno=0, qfile="", dgfile="", useOutlets=0, contcheck=1, cSol=1.0):
    """src/DinfConcLimAccum.cpp:61"""
    return _lib.load().tdx_tool_dinfconclimaccum(_b(angfile), _b(ctptfile), _b(dmfile), _b(datasrc), _b(lyrname), int(uselyrname), int(lyrno), _b(qfile), _b(dgfile),
                                                 int(useOutlets), int(contcheck), float(cSol))


def tlaccum(angfile, tsupfile, tcfile, tlafile, depfile, cinfile="", coutfile="", datasrc="", lyrname="", uselyrname=0, lyrno=0, useOutlets=0, usec=0, contcheck=1):
    """src/DinfTransLimAccum.cpp:61"""
    return _lib.load().tdx_tool_dinftranslimaccum(_b(angfile), _b(tsupfile), _b(tcfile), _b(tlafile), _b(depfile), _b(cinfile), _b(coutfile), _b(datasrc), _b(lyrname),
                                                  int(uselyrname), int(lyrno), int(useOutlets), int(usec), int(contcheck))
